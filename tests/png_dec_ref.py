"""Own restatements and writers for the PNG decoder's tests (numpy + zlib, nothing from the package under test):

    unfilter / filter_rows          the five row filters, both ways, for every bpp
    expand_bgr / expand_index       the expansion rules of DESIGN.md section 32
    png_bytes / adam7_png_bytes     a PNG writer with a chosen filter type per row, depth, colour type, IDAT split and extra chunks
    BitWriter, deflate_block, ...   a deflate writer with explicit tokens and explicit code lengths (zlib never emits a distance
                                    above 32506, a 15-bit code on demand, or an incomplete distance code)
    trace_inflate                   a slow inflate that reports what a stream contains (the census of the stream set)
    parse_inst_ref                  the reference's parse_inst on two index maps"""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def row_bytes(w, depth, ctype):
    return (w * CHANNELS[ctype] * depth + 7) // 8


def bpp_of(depth, ctype):
    return max(1, CHANNELS[ctype] * depth // 8)


# ---- the filters -----------------------------------------------------------------------------------------------------------------
def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def unfilter(raw, h, row, bpp):
    """raw: h * (row + 1) filtered bytes -> (h, row) uint8; a filter type above 4 is a ValueError"""
    raw = np.frombuffer(bytes(raw), np.uint8)
    assert raw.size == h * (row + 1), (raw.size, h, row)
    out = np.zeros((h, row), np.uint8)
    prev = [0] * row
    for y in range(h):
        ft = int(raw[y * (row + 1)])
        line = raw[y * (row + 1) + 1:(y + 1) * (row + 1)].tolist()
        if ft > 4:
            raise ValueError('filter type %d' % ft)
        if ft == 1:
            for x in range(bpp, row):
                line[x] = (line[x] + line[x - bpp]) & 255
        elif ft == 2:
            line = [(v + u) & 255 for v, u in zip(line, prev)]
        elif ft == 3:
            for x in range(row):
                line[x] = (line[x] + (((line[x - bpp] if x >= bpp else 0) + prev[x]) >> 1)) & 255
        elif ft == 4:
            for x in range(row):
                a = line[x - bpp] if x >= bpp else 0
                c = prev[x - bpp] if x >= bpp else 0
                line[x] = (line[x] + paeth(a, prev[x], c)) & 255
        out[y] = line
        prev = line
    return out


def filter_rows(rows, types, bpp):
    """rows (h, row) uint8, one filter type per row -> the filtered stream's bytes"""
    rows = np.asarray(rows, np.uint8)
    h, row = rows.shape
    out = bytearray()
    for y in range(h):
        cur = rows[y].astype(np.int32)
        up = rows[y - 1].astype(np.int32) if y else np.zeros(row, np.int32)
        a = np.concatenate([np.zeros(min(bpp, row), np.int32), cur[:-bpp]])[:row] if row > bpp else np.zeros(row, np.int32)
        c = np.concatenate([np.zeros(min(bpp, row), np.int32), up[:-bpp]])[:row] if row > bpp else np.zeros(row, np.int32)
        ft = int(types[y])
        if ft == 0:
            pred = np.zeros(row, np.int32)
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        elif ft == 4:
            p = a + up - c
            pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        else:
            pred = np.zeros(row, np.int32)          # (an invalid type, for the damaged files)
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


# ---- the expansion ---------------------------------------------------------------------------------------------------------------
def _samples(rows, w, depth, channels):
    """(h, row) uint8 -> (h, w, channels) int: the samples, of a 16-bit one the HIGH byte"""
    rows = np.asarray(rows, np.uint8)
    h = rows.shape[0]
    if depth < 8:
        bits = np.unpackbits(rows, axis=1)[:, :w * depth].reshape(h, w, depth)
        return (bits * (1 << np.arange(depth - 1, -1, -1))).sum(axis=2).reshape(h, w, 1)
    step = depth // 8
    return rows[:, :w * channels * step].reshape(h, w, channels, step)[:, :, :, 0].astype(np.int64)


def expand_bgr(rows, w, depth, ctype, palette=None):
    """what np.asarray(Image.open(f).convert('RGB'))[:, :, ::-1] gives; palette: (n, 3) uint8, n <= 256"""
    s = _samples(rows, w, depth, CHANNELS[ctype])
    if ctype == 3:
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(palette)] = palette
        rgb = pal[s[:, :, 0]]
    elif ctype in (0, 4):
        g = s[:, :, 0] * {1: 255, 2: 85, 4: 17, 8: 1, 16: 1}[depth]
        rgb = np.stack([g, g, g], axis=2)
    else:
        rgb = s[:, :, :3]
    return np.ascontiguousarray(rgb[:, :, ::-1].astype(np.uint8))


def expand_index(rows, w, depth, ctype):
    """what np.array(im.getdata(), np.uint8).reshape(h, w) gives for P and L images"""
    assert ctype in (0, 3)
    s = _samples(rows, w, depth, 1)[:, :, 0]
    return (s if ctype == 3 else s * {1: 255, 2: 85, 4: 17, 8: 1}[depth]).astype(np.uint8)


# ---- the container ---------------------------------------------------------------------------------------------------------------
def chunk(kind, body, crc=None):
    c = zlib.crc32(body, zlib.crc32(kind)) & 0xffffffff if crc is None else crc
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', c)


def png_bytes(w, h, depth, ctype, rows=None, types=None, palette=None, idat_split=None, before_idat=(), after_idat=(), level=6,
              interlace=0, zdata=None, iend=True):
    """rows (h, row) uint8 and one filter type per row (default 0) -> the file.  palette: (n, 3) uint8 -> a PLTE chunk; before_idat /
    after_idat: (kind, body) chunks; idat_split: bytes per IDAT chunk (default: one chunk); zdata: the zlib stream itself."""
    if zdata is None:
        types = [0] * h if types is None else types
        zdata = zlib.compress(filter_rows(rows, types, bpp_of(depth, ctype)), level)
    out = [SIGNATURE, chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, interlace))]
    if palette is not None:
        out.append(chunk(b'PLTE', np.asarray(palette, np.uint8).tobytes()))
    out += [chunk(k, b) for k, b in before_idat]
    step = idat_split or max(1, len(zdata))
    out += [chunk(b'IDAT', zdata[i:i + step]) for i in range(0, max(1, len(zdata)), step)]
    out += [chunk(k, b) for k, b in after_idat]
    if iend:
        out.append(chunk(b'IEND', b''))
    return b''.join(out)


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def adam7_png_bytes(pix, ctype):
    """pix (h, w, channels) uint8, 8 bits per sample -> a valid interlaced file (every pass with filter type 0)"""
    pix = np.asarray(pix, np.uint8)
    h, w = pix.shape[:2]
    raw = bytearray()
    for x0, y0, dx, dy in ADAM7:
        sub = pix[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        for r in sub.reshape(sub.shape[0], -1):
            raw.append(0)
            raw += r.tobytes()
    return png_bytes(w, h, 8, ctype, interlace=1, zdata=zlib.compress(bytes(raw)))


# ---- a deflate writer ------------------------------------------------------------------------------------------------------------
class BitWriter(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """nbits of value, the lowest first (headers, extra bits)"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: its first (most significant) bit first"""
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def length_symbol(L):
    """-> (symbol, extra bits, extra value)"""
    assert 3 <= L <= 258
    if L == 258:
        return 285, 0, 0
    if L <= 10:
        return 254 + L, 0, 0
    e = (L - 3).bit_length() - 3
    i = ((L - 3) >> e) - 4
    return 265 + 4 * (e - 1) + i, e, (L - 3) & ((1 << e) - 1)


def dist_symbol(D):
    assert 1 <= D <= 32768
    if D <= 4:
        return D - 1, 0, 0
    e = (D - 1).bit_length() - 2
    i = ((D - 1) >> e) - 2
    return 2 * (e + 1) + i, e, (D - 1) & ((1 << e) - 1)


def canonical(lens):
    """code lengths -> codes (RFC 1951 3.2.2)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = []
    for l in lens:
        codes.append(nxt[l] if l else 0)
        if l:
            nxt[l] += 1
    return codes


def fixed_lens():
    return [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32


def _tokens(bw, tokens, lit_lens, dist_lens):
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if t[0] == 'l':
            bw.code(lc[t[1]], lit_lens[t[1]])
        elif t[0] == 'm':
            s, e, v = length_symbol(t[1])
            bw.code(lc[s], lit_lens[s])
            bw.put(v, e)
            s, e, v = dist_symbol(t[2])
            assert dist_lens[s], ('no code for distance symbol', s)
            bw.code(dc[s], dist_lens[s])
            bw.put(v, e)
        elif t[0] == 'sym':          # a literal/length symbol as it is (286, 287: invalid)
            bw.code(lc[t[1]], lit_lens[t[1]])
        elif t[0] == 'dsym':         # a distance symbol as it is (30, 31: invalid), no extra bits
            bw.code(dc[t[1]], dist_lens[t[1]])
        elif t[0] == 'bits':
            bw.put(t[1], t[2])
        else:
            raise ValueError(t)
    bw.code(lc[256], lit_lens[256])


def fixed_block(bw, tokens, final):
    bw.put(final, 1)
    bw.put(1, 2)
    ll, dl = fixed_lens()
    _tokens(bw, tokens, ll, dl)


def stored_block(bw, data, final, nlen=None):
    bw.put(final, 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put((len(data) ^ 0xffff) if nlen is None else nlen, 16)
    bw.out += data


def rle_lengths(lens):
    """the code-length symbols of a sequence of lengths: (symbol, extra bits, extra value), with the repeats 16 / 17 / 18 running over
    the whole sequence (so from the literal/length lengths into the distance lengths where they continue)"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, 7, k - 11))
                run -= k
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, 2, k - 3))
                run -= k
            out += [(v, 0, 0)] * run
        i = j
    return out


# a complete code over all 19 code-length symbols: 13 codes of 4 bits and 6 of 5 bits
CLEN_LENS = [4] * 13 + [5] * 6


def dynamic_block(bw, tokens, final, lit_lens, dist_lens, clen_lens=None, nlen=None, ndist=None):
    """a dynamic block with the given code lengths (lit_lens: >= 257 entries, dist_lens: >= 1); returns the code-length symbols sent"""
    clen_lens = CLEN_LENS if clen_lens is None else clen_lens
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    bw.put(final, 1)
    bw.put(2, 2)
    bw.put((len(lit_lens) if nlen is None else nlen) - 257, 5)
    bw.put((len(dist_lens) if ndist is None else ndist) - 1, 5)
    bw.put(19 - 4, 4)
    for s in CLEN_ORDER:
        bw.put(clen_lens[s], 3)
    cc = canonical(clen_lens)
    syms = rle_lengths(lit_lens + dist_lens)
    for s, e, v in syms:
        bw.code(cc[s], clen_lens[s])
        bw.put(v, e)
    full_l = lit_lens + [0] * (288 - len(lit_lens))
    full_d = dist_lens + [0] * (32 - len(dist_lens))
    _tokens(bw, tokens, full_l, full_d)
    return syms


def zlib_wrap(body, data, header=b'\x78\x01', adler=None):
    return header + body + struct.pack('>I', zlib.adler32(data) & 0xffffffff if adler is None else adler)


def apply_tokens(tokens, prefix=b''):
    out = bytearray(prefix)
    for t in tokens:
        if t[0] == 'l':
            out.append(t[1])
        elif t[0] == 'm':
            for _ in range(t[1]):
                out.append(out[-t[2]])
    return bytes(out[len(prefix):])


# ---- a slow inflate that reports what it saw -------------------------------------------------------------------------------------
class _Bits(object):
    def __init__(self, data):
        self.d, self.pos = data, 0          # pos in bits

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _decoder(lens):
    codes = canonical(lens)
    return {(l, c): s for s, (l, c) in enumerate(zip(lens, codes)) if l}


def _decode(bits, table):
    code = 0
    for l in range(1, 16):
        code = (code << 1) | bits.take(1)
        s = table.get((l, code))
        if s is not None:
            return s
    raise ValueError('no such code')


def trace_inflate(stream):
    """a VALID zlib stream -> (its bytes, info): block types, counts, the length / distance / repeat symbols used, and the edge cases"""
    info = dict(types=set(), blocks=0, empty_stored=0, len_syms=set(), dist_syms=set(), rep_syms=set(), cross_repeat=False, max_code=0,
                no_dist_block=False, single_dist_block=False, overlap=False, d1_l258=False, dist_32768=False, prev_block=False,
                straddle=False)
    b = _Bits(stream)
    b.take(16)
    out = bytearray()
    while True:
        final, kind = b.take(1), b.take(2)
        info['types'].add(kind)
        info['blocks'] += 1
        start = len(out)
        if kind == 0:
            b.pos = (b.pos + 7) & ~7
            n = b.take(16)
            assert b.take(16) == n ^ 0xffff
            info['empty_stored'] += n == 0
            out += stream[b.pos >> 3:(b.pos >> 3) + n]
            b.pos += 8 * n
        else:
            if kind == 1:
                ll, dl = fixed_lens()
            else:
                nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for i in range(ncode):
                    cl[CLEN_ORDER[i]] = b.take(3)
                ct, lens = _decoder(cl), []
                while len(lens) < nlen + ndist:
                    s = _decode(b, ct)
                    if s < 16:
                        lens.append(s)
                        continue
                    info['rep_syms'].add(s)
                    rep = 3 + b.take(2) if s == 16 else 3 + b.take(3) if s == 17 else 11 + b.take(7)
                    if len(lens) < nlen < len(lens) + rep:
                        info['cross_repeat'] = True
                    lens += [lens[-1] if s == 16 else 0] * rep
                assert len(lens) == nlen + ndist
                ll, dl = lens[:nlen], lens[nlen:]
                info['max_code'] = max(info['max_code'], max(ll), max(dl))
                used = sum(1 for l in dl if l)
                info['no_dist_block'] |= used == 0
                info['single_dist_block'] |= used == 1
            lt, dt = _decoder(ll), _decoder(dl)
            while True:
                s = _decode(b, lt)
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                info['len_syms'].add(s)
                i = s - 257
                L = 258 if s == 285 else 3 + i if i < 8 else 3 + ((4 + (i & 3)) << ((i - 4) >> 2)) + b.take((i - 4) >> 2)
                d = _decode(b, dt)
                info['dist_syms'].add(d)
                D = 1 + d if d < 4 else 1 + ((2 + (d & 1)) << ((d >> 1) - 1)) + b.take((d >> 1) - 1)
                assert D <= len(out)
                info['overlap'] |= D < L
                info['d1_l258'] |= D == 1 and L == 258
                info['dist_32768'] |= D == 32768
                info['prev_block'] |= len(out) - D < start
                info['straddle'] |= len(out) < 32768 < len(out) + L
                for _ in range(L):
                    out.append(out[-D])
        if final:
            break
    b.pos = (b.pos + 7) & ~7
    assert struct.unpack('>I', stream[b.pos >> 3:(b.pos >> 3) + 4])[0] == zlib.adler32(bytes(out)) & 0xffffffff
    assert (b.pos >> 3) + 4 == len(stream)
    return bytes(out), info


# ---- the stream set of the inflate tests -----------------------------------------------------------------------------------------
def _hand_fixed(tokens, prefix_tokens=()):
    bw = BitWriter()
    fixed_block(bw, list(prefix_tokens) + list(tokens), 1)
    data = apply_tokens(list(prefix_tokens) + list(tokens))
    return zlib_wrap(bw.bytes(), data), data


def stream_set():
    """-> [(name, zlib stream, the bytes it inflates to)]: what tests/test_png_dec_cpu.py censuses and both inflate tests decode"""
    rng = np.random.default_rng(5)
    out = []

    def add(name, stream, data):
        out.append((name, stream, bytes(data)))

    def z(name, data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
        parts, at = [], 0
        for f in flush_at:
            parts += [c.compress(data[at:f]), c.flush(zlib.Z_FULL_FLUSH)]
            at = f
        parts += [c.compress(data[at:]), c.flush()]
        add(name, b''.join(parts), data)

    text = bytes(rng.integers(97, 105, 3000).astype(np.uint8))
    z('empty', b'')
    z('one_byte', b'\x2a')
    z('stored', bytes(rng.integers(0, 256, 700).astype(np.uint8)), level=0)
    z('fixed', b'abcabcabcabd')
    z('dynamic', text * 3)
    z('flushes', text + bytes(range(256)) * 4 + text[::-1], flush_at=(1000, 1000, 2500))          # (two flushes in a row: empty blocks)
    z('huffman_only', bytes(np.clip(rng.normal(128, 6, 5000), 0, 255).astype(np.uint8)), strategy=zlib.Z_HUFFMAN_ONLY)
    z('rle', b''.join(bytes([int(v)]) * int(n) for v, n in zip(rng.integers(0, 256, 300), rng.integers(1, 400, 300))), strategy=zlib.Z_RLE)
    low = np.cumsum(rng.integers(-2, 3, 40000)).astype(np.uint8).tobytes()
    for n in (32767, 32768, 32769, 65537):
        z('lowpass_%d' % n, low[:n] if n <= len(low) else (low + low)[:n], level=6 if n != 32769 else 1)
    z('noise_32769', bytes(rng.integers(0, 256, 32769).astype(np.uint8)), level=9)
    # every length code and every distance code, by hand with the fixed code: literals first, so that every distance is in reach
    base = [('l', int(v)) for v in rng.integers(0, 256, 700)]
    toks = list(base)
    for s in range(257, 286):
        L = 258 if s == 285 else next(L for L in range(3, 259) if length_symbol(L)[0] == s)
        toks.append(('m', L, 1 + (s % 7)))
        toks.append(('m', 258 if s == 285 else min(258, L + (1 << length_symbol(L)[1]) - 1), 300 + s))          # the code's largest length
    produced = len(apply_tokens(toks))
    for d in range(30):
        D = next(D for D in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                             6145, 8193, 12289, 16385, 24577) if dist_symbol(D)[0] == d)
        while produced < D:
            toks.append(('m', 258, 1))
            produced += 258
        toks.append(('m', 3 + d, D))
        produced += 3 + d
    add('all_codes', *_hand_fixed(toks))
    # distances zlib never emits: exactly 32768 (with the longest match, so that source and destination share ring slots), and near it
    toks = [('l', int(v)) for v in rng.integers(0, 256, 300)]
    produced = 300
    while produced < 32768 - 100:
        toks.append(('m', 258, 300))
        produced += 258
    toks.append(('m', 258, 1))          # straddles 32768; distance 1, length 258
    produced += 258
    toks += [('l', 7)] * (32768 + 40 - produced) if produced < 32768 + 40 else []
    produced = len(apply_tokens(toks))
    toks.append(('m', 258, 32768 if produced >= 32768 else produced))
    toks.append(('m', 258, 32767))
    toks.append(('m', 258, 32768 - 64))
    toks.append(('m', 257, 32768 - 63))
    toks.append(('m', 200, 32768))
    add('far', *_hand_fixed(toks))
    # two blocks: the second one's first match reaches into the bytes of the first; then an empty stored block and a last fixed one
    bw = BitWriter()
    first = [('l', int(v)) for v in rng.integers(0, 256, 50)]
    fixed_block(bw, first, 0)
    second = [('m', 40, 45), ('l', 1), ('m', 9, 2)]
    fixed_block(bw, second, 0)
    stored_block(bw, b'', 0)
    stored_block(bw, b'xyz', 0)
    fixed_block(bw, [], 1)
    data = apply_tokens(first + second) + b'xyz'
    add('two_blocks', zlib_wrap(bw.bytes(), data), data)
    # dynamic blocks by hand: a 15-bit code; a repeat that runs from the literal/length lengths into the distance lengths
    lit = [0] * 257
    for k, s in enumerate([65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77, 78]):
        lit[s] = k + 1                  # lengths 1 .. 14
    lit[79] = 15
    lit[256] = 15
    toks = [('l', 65)] * 9 + [('l', s) for s in range(65, 80)] + [('l', 79), ('l', 65)]
    bw = BitWriter()
    dynamic_block(bw, toks, 1, lit, [0])                  # no distance code at all
    add('deep_code', zlib_wrap(bw.bytes(), apply_tokens(toks)), apply_tokens(toks))
    # all 286 literal/length symbols: 226 codes of 8 bits and 60 of 9 (226 * 2 + 60 = 512: complete)
    lit_all = [8] * 226 + [9] * 60
    # the same with the last 16 length symbols unused (242 * 2 + 28 = 512), so that the lengths END in a run of zeros, and five unused
    # distance symbols FIRST: one repeat symbol (18) carries the 21 zeros across the boundary
    lit_z = [8] * 242 + [9] * 28 + [0] * 16
    dist_z = [0, 0, 0, 0, 0, 1, 1]
    toks = [('l', int(v)) for v in rng.integers(0, 226, 400)] + [('m', 10, 7), ('m', 4, 9), ('l', 3)]
    bw = BitWriter()
    dynamic_block(bw, toks, 1, lit_z, dist_z)
    add('cross_repeat', zlib_wrap(bw.bytes(), apply_tokens(toks)), apply_tokens(toks))
    # ONE distance code of length 1: the incomplete set zlib accepts (this project's own encoder writes it)
    toks = [('l', 5), ('m', 258, 1), ('m', 17, 1), ('l', 9), ('m', 3, 1)]
    bw = BitWriter()
    dynamic_block(bw, toks, 1, lit_all, [1])
    add('single_distance', zlib_wrap(bw.bytes(), apply_tokens(toks)), apply_tokens(toks))
    return out


def damaged_set():
    """-> [(name, stream, capacity, the one status bit)]"""
    good = zlib.compress(bytes(range(200)) * 3, 6)
    data = bytes(range(200)) * 3
    out = []
    out.append(('cm', bytes([0x79, 0x9c ^ 0]) + good[2:], 600, 1))
    hdr = 0x88 << 8
    out.append(('window', struct.pack('>H', hdr + (31 - hdr % 31) % 31) + good[2:], 600, 1))
    hdr = (0x78 << 8) | 0x20
    out.append(('fdict', struct.pack('>H', hdr + (31 - hdr % 31) % 31) + good[2:], 600, 1))
    out.append(('fcheck', b'\x78\x9d' + good[2:], 600, 1))
    bw = BitWriter()
    bw.put(1, 1)
    bw.put(3, 2)
    out.append(('block_type', zlib_wrap(bw.bytes(), b''), 600, 2))
    bw = BitWriter()
    stored_block(bw, b'abcd', 1, nlen=0x1234)
    out.append(('stored_len', zlib_wrap(bw.bytes(), b'abcd'), 600, 4))
    bw = BitWriter()                                                 # over-subscribed: 258 codes of 8 bits
    dynamic_block(bw, [], 1, [8] * 258, [1, 1])
    out.append(('oversubscribed', zlib_wrap(bw.bytes(), b''), 600, 8))
    bw = BitWriter()
    dynamic_block(bw, [], 1, [8] * 200 + [0] * 56 + [8], [1, 1])   # incomplete literal/length set of more than one code
    out.append(('incomplete_lit', zlib_wrap(bw.bytes(), b''), 600, 8))
    lit_ok = [8] * 255 + [9, 9]                                    # symbols 0 .. 254 (8), 255 and 256 (9): complete
    bw = BitWriter()
    dynamic_block(bw, [], 1, lit_ok, [2, 2])                       # two distance codes of length 2: incomplete, longer than 1
    out.append(('incomplete_dist', zlib_wrap(bw.bytes(), b''), 600, 8))
    bw = BitWriter()
    dynamic_block(bw, [], 1, [8] * 255 + [9, 0] + [9], [1, 1])          # no end-of-block code
    out.append(('no_eob', zlib_wrap(bw.bytes(), b''), 600, 8))
    bw = BitWriter()                                                 # a repeat (16) with no length before it
    bw.put(1, 1); bw.put(2, 2); bw.put(0, 5); bw.put(0, 5); bw.put(15, 4)
    for s in CLEN_ORDER:
        bw.put(CLEN_LENS[s], 3)
    cc = canonical(CLEN_LENS)
    bw.code(cc[16], CLEN_LENS[16]); bw.put(0, 2)
    out.append(('repeat_first', zlib_wrap(bw.bytes() + b'\0' * 8, b''), 600, 8))
    bw = BitWriter()                                                 # HLIT = 30: 287 literal/length codes
    bw.put(1, 1); bw.put(2, 2); bw.put(30, 5); bw.put(0, 5); bw.put(15, 4)
    out.append(('too_many', zlib_wrap(bw.bytes() + b'\0' * 8, b''), 600, 8))
    for s in (286, 287):
        bw = BitWriter()
        fixed_block(bw, [('l', 1), ('sym', s)], 1)
        out.append(('symbol_%d' % s, zlib_wrap(bw.bytes(), b'\x01'), 600, 16))
    for d in (30, 31):
        bw = BitWriter()
        fixed_block(bw, [('l', 1), ('l', 2), ('l', 3), ('sym', 257), ('dsym', d)], 1)
        out.append(('distance_%d' % d, zlib_wrap(bw.bytes(), b'\x01\x02\x03'), 600, 16))
    bw = BitWriter()                                                 # the one distance code has length 1: the other bit is no code
    lit_z = [8] * 242 + [9] * 28 + [0] * 16
    dynamic_block(bw, [('l', 5), ('sym', 257), ('bits', 1, 1)], 1, lit_z, [1])
    out.append(('unassigned_code', zlib_wrap(bw.bytes(), b'\x05'), 600, 16))
    bw = BitWriter()
    fixed_block(bw, [('l', 1), ('l', 2), ('m', 3, 3)], 1)           # distance 3 at position 2
    out.append(('far_distance', zlib_wrap(bw.bytes(), b''), 600, 32))
    out.append(('truncated', good[:len(good) // 2], 600, 64))
    out.append(('no_adler', good[:-2], 600, 64))
    out.append(('nothing', b'', 600, 64))
    out.append(('capacity', good, len(data) - 1, 128))
    out.append(('capacity_0', good, 0, 128))
    bw = BitWriter()
    fixed_block(bw, [('l', 1)] + [('m', 258, 1)] * 3, 1)
    out.append(('capacity_match', zlib_wrap(bw.bytes(), b'\x01' * 775), 700, 128))
    bw = BitWriter()
    stored_block(bw, bytes(500), 1)
    out.append(('capacity_stored', zlib_wrap(bw.bytes(), bytes(500)), 300, 128))
    out.append(('adler', good[:-1] + bytes([good[-1] ^ 1]), 600, 256))
    out.append(('trailing', good + b'\0', 600, 512))
    return out


# ---- parse_inst ------------------------------------------------------------------------------------------------------------------
def parse_inst_ref(obj, cls):
    """the reference's parse_inst (lib/dataset/pascal_voc_eval.py:275-318) on the two index maps, restated"""
    obj, cls = np.asarray(obj, np.uint8), np.asarray(cls, np.uint8)
    record = []
    for k in np.unique(obj):
        if k == 0:
            continue
        r, c = np.where(obj == k)
        bound = np.array([c.min(), r.min(), c.max(), r.max()], dtype=int)
        mask = obj[bound[1]:bound[3] + 1, bound[0]:bound[2] + 1] == k
        classes = np.unique(cls[bound[1]:bound[3] + 1, bound[0]:bound[2] + 1][mask])
        assert classes.shape[0] == 1
        record.append({'mask': mask, 'mask_cls': classes[0], 'mask_bound': bound})
    return record


# ---- reading a file back, and the files of the decoder's tests --------------------------------------------------------------------
def read_png(data):
    """-> dict(w, h, depth, ctype, lace, palette (n, 3) or None, idat, kinds): a plain chunk walk (valid files only)"""
    assert data[:8] == SIGNATURE
    pos, idat, kinds, palette, head = 8, [], [], None, None
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        kinds.append(kind)
        if kind == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif kind == b'PLTE':
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b'IDAT':
            idat.append(body)
        pos += 12 + n
    return dict(w=head[0], h=head[1], depth=head[2], ctype=head[3], lace=head[6], palette=palette, idat=b''.join(idat), kinds=kinds)


def decode_ref(data, mode='bgr'):
    """the restatement of the whole decoder: chunk walk, zlib, unfilter, expansion"""
    f = read_png(data)
    row = row_bytes(f['w'], f['depth'], f['ctype'])
    rows = unfilter(zlib.decompress(f['idat']), f['h'], row, bpp_of(f['depth'], f['ctype']))
    if mode == 'index':
        return expand_index(rows, f['w'], f['depth'], f['ctype'])
    return expand_bgr(rows, f['w'], f['depth'], f['ctype'], f['palette'])


# colour type, depth: what the device decodes (16-bit grey, with or without alpha, is a fallback)
COMBOS = ((0, 1), (0, 2), (0, 4), (0, 8), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (6, 8), (6, 16))
SIZES = ((1, 1), (1, 70), (70, 1), (9, 13), (130, 67))          # (h, w)
FRONT_SIZES = ((63, 65), (64, 64), (65, 63), (129, 2), (64, 1), (129, 1))          # the edges of a 64-lane front


def random_rows(rng, h, w, depth, ctype, smooth=False):
    row = row_bytes(w, depth, ctype)
    if smooth:          # neighbouring bytes close to each other: Average and Paeth predictions near the 0 / 255 wrap
        return (np.cumsum(rng.integers(-3, 4, (h, row)), axis=1) + rng.integers(0, 256, (h, 1))).astype(np.uint8)
    return rng.integers(0, 256, (h, row)).astype(np.uint8)


def palette_for(rng, depth, short=False):
    n = 1 << depth
    if short:
        n = max(1, n // 2 - 1)
    return rng.integers(0, 256, (n, 3)).astype(np.uint8)


def matrix_files(sizes=SIZES, combos=COMBOS, seed=11):
    """-> [(name, the file's bytes)]: colour type x depth x size, and five files of each whose rows cycle through the five filters
    from a different start (so every filter meets the first row)"""
    rng = np.random.default_rng(seed)
    out = []
    for ctype, depth in combos:
        for h, w in sizes:
            rows = random_rows(rng, h, w, depth, ctype, smooth=(h * w) % 2 == 0)
            pal = palette_for(rng, depth) if ctype == 3 else None
            for k in range(5):
                types = [(y + k) % 5 for y in range(h)]
                out.append(('c%d_d%d_%dx%d_f%d' % (ctype, depth, h, w, k), png_bytes(w, h, depth, ctype, rows, types, palette=pal)))
    return out


def special_files(seed=12):
    """-> [(name, bytes)]: PIL-saved files, a file of 1-byte IDATs, tRNS / gAMA / a short PLTE / a PLTE in a true-colour file"""
    import io
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    pic = (np.cumsum(rng.integers(-4, 5, (40, 57, 3)), axis=1) + 128).astype(np.uint8)

    def saved(im, **kw):
        buf = io.BytesIO()
        im.save(buf, 'PNG', **kw)
        return buf.getvalue()
    out.append(('pil_default', saved(Image.fromarray(pic))))
    out.append(('pil_optimize', saved(Image.fromarray(pic), optimize=True)))
    out.append(('pil_level0', saved(Image.fromarray(pic), compress_level=0)))
    out.append(('pil_level1', saved(Image.fromarray(pic), compress_level=1)))
    out.append(('pil_grey', saved(Image.fromarray(pic[:, :, 0]))))
    out.append(('pil_palette', saved(Image.fromarray(pic).quantize(17))))
    out.append(('pil_rgba', saved(Image.fromarray(np.dstack([pic, pic[:, :, :1]])))))
    out.append(('pil_bilevel', saved(Image.fromarray(pic[:, :, 0] > 128))))
    rows = random_rows(rng, 12, 19, 8, 2)
    out.append(('idat_1byte', png_bytes(19, 12, 8, 2, rows, [4] * 12, idat_split=1)))
    out.append(('rgb_trns_gama', png_bytes(19, 12, 8, 2, rows, [3] * 12, before_idat=[(b'gAMA', struct.pack('>I', 45455)),
                                                                                     (b'tRNS', bytes(rows[0, :3].astype(np.uint16).byteswap().tobytes()))])))
    out.append(('rgb_with_plte', png_bytes(19, 12, 8, 2, rows, [1] * 12, palette=palette_for(rng, 4))))
    g = random_rows(rng, 7, 33, 4, 0)
    out.append(('grey_trns', png_bytes(33, 7, 4, 0, g, [2] * 7, before_idat=[(b'tRNS', b'\x00\x03'), (b'sRGB', b'\x00')])))
    for depth in (2, 4, 8):
        p = random_rows(rng, 9, 21, depth, 3)
        pal = palette_for(rng, depth, short=True)
        out.append(('short_plte_d%d' % depth, png_bytes(21, 9, depth, 3, p, [(y * 3) % 5 for y in range(9)], palette=pal)))
        out.append(('plte_trns_d%d' % depth, png_bytes(21, 9, depth, 3, p, [4] * 9, palette=palette_for(rng, depth),
                                                       before_idat=[(b'tRNS', bytes([0, 128, 255]))])))
    return out


def pil_bgr(data):
    import io
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[:, :, ::-1])


def pil_index(data):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    return np.array(im.getdata(), np.uint8).reshape(im.size[1], im.size[0])


def voc_maps(seed=13):
    """-> [(object map, class map)] of (1, 1), (37, 53) and (375, 500): an id at 255, an instance of one pixel, one that touches all
    four borders, two interleaved instances"""
    rng = np.random.default_rng(seed)
    out = []
    out.append((np.array([[255]], np.uint8), np.array([[255]], np.uint8)))
    for h, w in ((37, 53), (375, 500)):
        obj, cls = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        obj[0, :] = obj[-1, :] = obj[:, 0] = obj[:, -1] = 3          # a frame: touches all four borders
        obj[5:20:2, 4:30] = 1                                        # two instances in alternating rows
        obj[6:20:2, 4:30] = 2
        obj[h // 2, w // 2] = 7                                      # one pixel
        obj[h - 9:h - 3, w - 12:w - 2] = 255
        blob = rng.integers(0, 4, (10, 14)) == 0
        obj[22:32, 30:44][blob] = 9
        for k, c in ((1, 15), (2, 15), (3, 20), (7, 1), (9, 8), (255, 255)):
            cls[obj == k] = c
        out.append((obj, cls))
    return out


# ---- the stand-alone host program over sniper_amd/csrc/inflate_code.h -------------------------------------------------------------
def compile_inflate_program(out_dir, sanitize=False):
    """tests/png_inflate_main.cpp -> the program's path; sanitize: with -fsanitize=address,undefined (a program of its own: nothing
    is loaded into Python)"""
    import os
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        from sniper_amd.build import _hipcc
        cxx = _hipcc()
    exe = os.path.join(str(out_dir), 'png_inflate_main' + ('_san' if sanitize else ''))
    flags = ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitize else ['-O1']
    subprocess.run([cxx] + flags + ['-std=c++17', '-Wall', os.path.join(here, 'png_inflate_main.cpp'), '-o', exe], check=True)
    return exe


def run_inflate_program(exe, cases):
    """cases: [(stream, capacity)] -> [(status, bytes produced, guard untouched, the output)]"""
    import subprocess
    text = ''.join('%d %s\n' % (cap, bytes(s).hex() or '-') for s, cap in cases)
    r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert len(rows) == len(cases), (len(rows), len(cases))
    return [(int(f[0]), int(f[1]), f[2] == '1', b'' if f[3] == '-' else bytes.fromhex(f[3])) for f in rows]
