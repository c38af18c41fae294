"""The numpy restatement of the JPEG decoder PIL runs (libjpeg, slow-integer IDCT, fancy upsampling), all in integers: what
sniper_amd/csrc/jpeg_decode.hip computes.  decode_bgr(data) is compared bit for bit with PIL in tests/test_jpeg_cpu.py.

    coefficients(head, data)      entropy decoding: per block 64 values in natural order, DC summed, blocks in the order of the scan
    idct(blocks, q)               dequantise and invert, columns first
    upsample_h2v1 / _h2v2         the two chroma upsamplers
    colour(y, cb, cr)             YCbCr -> B, G, R"""
import numpy as np

from sniper_amd.jpeg import ZIGZAG, parse_jpeg


def build_codes(dht):
    """one DHT table (16 counts, then values) -> {(length, code): value}"""
    codes, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(int(dht[l - 1])):
            codes[(l, code)] = int(dht[16 + k])
            code += 1
            k += 1
        code <<= 1
    return codes


class Bits(object):
    def __init__(self, seg):
        raw = np.frombuffer(bytes(seg), np.uint8)
        stuffed = np.zeros(raw.size, bool)
        stuffed[1:] = (raw[1:] == 0) & (raw[:-1] == 0xff)
        self.raw = np.flatnonzero(~stuffed)                 # the index in the segment of every data byte
        self.n = raw.size
        self.d = bytes(raw[~stuffed])
        self.acc, self.cnt, self.i = 0, 0, 0

    def rawpos(self):
        """the bit position of the next bit inside the segment, stuffed bytes counted"""
        if self.cnt:
            return int(self.raw[self.i - 1]) * 8 + 8 - self.cnt
        return int(self.raw[self.i]) * 8 if self.i < len(self.d) else self.n * 8

    def bit(self):
        if self.cnt == 0:
            if self.i >= len(self.d):
                raise ValueError('the segment ran out of bits')
            self.acc, self.cnt = self.d[self.i], 8
            self.i += 1
        self.cnt -= 1
        return (self.acc >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, codes):
        code = 0
        for l in range(1, 17):
            code = (code << 1) | self.bit()
            if (l, code) in codes:
                return codes[(l, code)]
        raise ValueError('no code matches')


def extend(v, t):
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def coefficients(head, data, starts=None):
    """-> (n_mcu * bpm, 64) int32: the blocks in scan order (per MCU hs * vs luma blocks row-major, then one block per chroma
    component), natural order inside a block, not yet dequantised, DC values summed per component inside each restart interval;
    starts: a list that receives the bit position in the file of every symbol (a code with its extra bits)"""
    tabs = [build_codes(t) for t in head['dht']]
    bpm, nluma, ri, n_mcu = head['bpm'], head['hs'] * head['vs'], head['ri'], head['n_mcu']
    out = np.zeros((n_mcu * bpm, 64), np.int32)
    for s, (a, b) in enumerate(zip(head['seg_first'], head['seg_end'])):
        rd = Bits(data[int(a):int(b)])
        mcus = range(s * ri, min(n_mcu, (s + 1) * ri)) if ri else range(n_mcu)
        pred = [0, 0, 0]
        for m in mcus:
            for j in range(bpm):
                c = 0 if j < nluma else 1 + j - nluma
                dc, ac = tabs[(head['sel'] >> (2 * c)) & 1], tabs[2 + ((head['sel'] >> (2 * c + 1)) & 1)]
                blk = out[m * bpm + j]
                if starts is not None:
                    starts.append(int(a) * 8 + rd.rawpos())
                t = rd.symbol(dc)
                pred[c] += extend(rd.bits(t), t)
                blk[0] = pred[c]
                k = 1
                while k < 64:
                    if starts is not None:
                        starts.append(int(a) * 8 + rd.rawpos())
                    rs = rd.symbol(ac)
                    r, sz = rs >> 4, rs & 15
                    if sz == 0:
                        if r != 15:
                            break
                        k += 16
                        continue
                    k += r
                    blk[ZIGZAG[k]] = extend(rd.bits(sz), sz)
                    k += 1
    return out


def _pass(i, n):
    """the 1-D pass on i[0..7] (arrays), each output (x + 2^(n-1)) >> n"""
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    outs = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)
    return [(x + (1 << (n - 1))) >> n for x in outs]


def idct(blocks, q):
    """blocks (n, 64) coefficients in natural order, q (64,) -> (n, 8, 8) uint8 samples"""
    x = (np.asarray(blocks, np.int32) * np.asarray(q, np.int32)[None, :]).astype(np.int32).reshape(-1, 8, 8)
    cols = np.stack(_pass([x[:, r, :] for r in range(8)], 11), axis=1)           # down the columns: the inputs are the 8 rows
    rows = np.stack(_pass([cols[:, :, c] for c in range(8)], 18), axis=2)
    rows = ((rows + 512) & 1023) - 512
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def planes(head, coef):
    """-> per component the (mcuy * v * 8, mcux * h * 8) plane of samples, the MCU padding included"""
    hs, vs, mcux, mcuy, bpm = head['hs'], head['vs'], head['mcux'], head['mcuy'], head['bpm']
    out = []
    for c in range(head['ncomp']):
        h, v = (hs, vs) if c == 0 else (1, 1)
        pl = np.zeros((mcuy, v, 8, mcux, h, 8), np.uint8)
        for by in range(v):
            for bx in range(h):
                j = by * hs + bx if c == 0 else hs * vs + c - 1
                pl[:, by, :, :, bx, :] = idct(coef[j::bpm], head['qtab'][c]).reshape(mcuy, mcux, 8, 8).transpose(0, 2, 1, 3)
        out.append(pl.reshape(mcuy * v * 8, mcux * h * 8))
    return out


def upsample_h2v1(p):
    """(h, cw) -> (h, 2 * cw)"""
    p = p.astype(np.int32)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.zeros((p.shape[0], 2 * p.shape[1]), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def upsample_h2v2(p):
    """(ch, cw) -> (2 * ch, 2 * cw)"""
    p = p.astype(np.int32)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.zeros((2 * p.shape[0], 2 * p.shape[1]), np.int32)
    for par, nb in ((0, up), (1, down)):
        t = 3 * p + nb
        left = np.concatenate([t[:, :1], t[:, :-1]], axis=1)
        right = np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
        out[par::2, 0::2] = (3 * t + left + 8) >> 4
        out[par::2, 1::2] = (3 * t + right + 7) >> 4
    return out


def colour(y, cb, cr):
    """-> (H, W, 3) uint8 B, G, R"""
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], axis=2), 0, 255).astype(np.uint8)


def decode_bgr(data, head=None):
    head = head or parse_jpeg(data)
    if 'fallback' in head:
        raise ValueError('not decoded here: ' + head['fallback'])
    H, W, hs, vs = head['H'], head['W'], head['hs'], head['vs']
    pl = planes(head, coefficients(head, data))
    y = pl[0][:H, :W]
    if head['ncomp'] == 1:
        return np.stack([y, y, y], axis=2)
    cw, ch = -(-W // hs), -(-H // vs)
    chroma = []
    for p in pl[1:]:
        p = p[:ch, :cw]                    # the component's own size: the padding is never read
        if hs == 2 and cw <= 2:
            p = np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)          # libjpeg keeps the triangle filter for planes wider than 2
        elif hs == 2 and vs == 2:
            p = upsample_h2v2(p)
        elif hs == 2:
            p = upsample_h2v1(p)
        chroma.append(p[:H, :W])
    return colour(y, chroma[0], chroma[1])


def entropy_job(head, data, mode='seq', sub=64, want_coef=True):
    """the five lines tests/jpeg_entropy_main.cpp reads for one file"""
    n_mcu, ri, bpm = head['n_mcu'], head['ri'], head['bpm']
    segs = []
    for s, (a, b) in enumerate(zip(head['seg_first'], head['seg_end'])):
        mcus = min(ri, n_mcu - s * ri) if ri else n_mcu
        segs += [int(a), int(b), mcus * bpm]
    return ['%s %d %d %d %d %d %d' % (mode, bpm, head['hs'] * head['vs'], head['sel'], sub, len(head['seg_first']), 1 if want_coef else 0),
            bytes(head['dht'].reshape(-1)).hex(), bytes(data).hex() or '-', ' '.join(str(v) for v in segs)]
