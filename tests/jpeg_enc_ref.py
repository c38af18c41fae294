"""The JPEG encoder restated in numpy / Python integers: baseline, the scaled Annex K quantisation tables,
libjpeg's edge rule and downsampling, its slow-integer forward DCT, the Annex K Huffman tables, one interleaved scan.  encode() is
byte for byte what PIL (libjpeg-turbo) writes for Image.save(..., 'JPEG', quality=q, subsampling=s); the kernels of
csrc/jpeg_encode.hip are compared with its stages."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
QUANT_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
              18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
QUANT_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
            0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
            0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
            0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
            0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
            0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
            0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
            0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
              0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
              0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
              0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
              0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
              0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
              0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
              0xfa])
SAMPLINGS = {'4:2:0': (2, 2), '4:2:2': (2, 1), '4:4:4': (1, 1)}
PIL_SUBSAMPLING = {'4:2:0': 2, '4:2:2': 1, '4:4:4': 0}


def quant_table(base, quality):
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(255, max(1, (b * s + 50) // 100)) for b in base]


def huff_codes(table):
    """(counts of the lengths 1 .. 16, values) -> {value: (code, length)}"""
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(table[0][length - 1]):
            out[table[1][k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _fdct_1d(d, first, dtype):
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    c = lambda v: dtype(v)
    descale = lambda x, n: (x + c(1 << (n - 1))) >> c(n)
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) * c(4), (t10 - t11) * c(4)
    else:
        o[0], o[4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * c(4433)
    o[2], o[6] = descale(z1 + t13 * c(6270), n), descale(z1 - t12 * c(15137), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * c(9633)
    t4, t5, t6, t7 = t4 * c(2446), t5 * c(16819), t6 * c(25172), t7 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return o


def fdct(blocks, dtype=np.int64):
    """blocks (..., 8, 8) samples minus 128 -> 8 x the DCT, rows first, then columns; dtype: the integers it is computed in"""
    b = np.asarray(blocks).astype(dtype)
    with np.errstate(over='raise'):
        rows = np.stack(_fdct_1d([b[..., :, i] for i in range(8)], True, dtype), -1)
        return np.stack(_fdct_1d([rows[..., i, :] for i in range(8)], False, dtype), -2)


def quantise(coef, table):
    d = np.array(table, np.int64).reshape(8, 8) * 8
    t = (np.abs(coef) + (d >> 1)) // d
    return np.where(coef < 0, -t, t)


def _pad(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode='edge')


def _components(pic):
    if pic.ndim == 2:
        return [pic.astype(np.int64)]
    r, g, b = [pic[..., i].astype(np.int64) for i in range(3)]
    return [(19595 * r + 38470 * g + 7471 * b + 32768) >> 16,
            (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16,
            (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16]


def geometry(h, w, subsampling, grey):
    hs, vs = (1, 1) if grey else SAMPLINGS[subsampling]
    return hs, vs, -(-w // (8 * hs)), -(-h // (8 * vs))


def component_samples(pic, subsampling='4:2:0'):
    """-> per component: the (8 * hb, 8 * wb) samples the transform sees (edges extended, chroma downsampled)"""
    H, W = pic.shape[:2]
    hs, vs, _, _ = geometry(H, W, subsampling, pic.ndim == 2)
    out = []
    for ci, p in enumerate(_components(pic)):
        h, v = (hs, vs) if ci == 0 else (1, 1)
        cw, ch = -(-W * h // hs), -(-H * v // vs)
        wb, hb = -(-cw // 8), -(-ch // 8)
        if ci and (hs > 1 or vs > 1):
            p = _pad(p, -(-H // vs) * vs, wb * 8 * hs)          # the row to 8 * wb * hs samples, the rows to a multiple of vs only
            if vs == 2:
                bias = np.where(np.arange(wb * 8) % 2 == 0, 1, 2)
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
            else:
                bias = np.where(np.arange(wb * 8) % 2 == 0, 0, 1)
                p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append(_pad(p, hb * 8, wb * 8))                     # (after downsampling: the last DOWNSAMPLED row repeated)
    return out


def blocks(pic, quality=75, subsampling='4:2:0', want_dummy=False):
    """-> (n_blocks, 64) int64: the quantised blocks in scan order, zig-zag order inside a block, dummies resolved, DC not differenced"""
    H, W = pic.shape[:2]
    grey = pic.ndim == 2
    hs, vs, mw, mh = geometry(H, W, subsampling, grey)
    planes = []
    for ci, p in enumerate(component_samples(pic, subsampling)):
        h, v = (hs, vs) if ci == 0 else (1, 1)
        hb, wb = p.shape[0] // 8, p.shape[1] // 8
        q = quantise(fdct(p.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3) - 128), quant_table(QUANT_LUMA if ci == 0 else QUANT_CHROMA, quality))
        full = np.zeros((mh * v, mw * h, 64), np.int64)
        real = np.zeros((mh * v, mw * h), bool)
        full[:hb, :wb] = q.reshape(hb, wb, 64)[:, :, ZIGZAG]
        real[:hb, :wb] = True
        planes.append((full, real, h, v))
    out, dummy = [], []
    for my in range(mh):
        for mx in range(mw):
            last_dc = 0
            for full, real, h, v in planes:
                for by in range(v):
                    for bx in range(h):
                        y, x = my * v + by, mx * h + bx
                        blk = full[y, x] if real[y, x] else np.array([last_dc] + [0] * 63, np.int64)
                        dummy.append((not real[y, x], bx, by))
                        last_dc = int(blk[0])
                        out.append(blk)
    out = np.array(out, np.int64).reshape(-1, 64)
    return (out, dummy) if want_dummy else out


def block_components(n_blocks, pic_is_grey, subsampling='4:2:0'):
    """the component (0, 1, 2) of every block of a scan"""
    if pic_is_grey:
        return np.zeros(n_blocks, np.int64)
    hs, vs = SAMPLINGS[subsampling]
    unit = [0] * (hs * vs) + [1, 2]
    return np.array(unit * (n_blocks // len(unit)), np.int64)


def scan(blks, comps, want_bits=False):
    """blocks (n, 64) and their components -> the entropy-coded bytes (stuffed, filled); want_bits: also the bits of every block"""
    tabs = [(huff_codes(DC_LUMA), huff_codes(AC_LUMA)), (huff_codes(DC_CHROMA), huff_codes(AC_CHROMA))]
    acc = cnt = 0
    out = bytearray()
    sizes = []
    total = [0]

    def put(code, length):
        nonlocal acc, cnt
        total[0] += length
        acc = (acc << length) | code
        cnt += length
        while cnt >= 8:
            byte = (acc >> (cnt - 8)) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
            cnt -= 8
        acc &= (1 << cnt) - 1
    pred = [0, 0, 0]
    for blk, ci in zip(blks, comps):
        before = total[0]
        dct, act = tabs[0 if ci == 0 else 1]
        d = int(blk[0]) - pred[ci]
        pred[ci] = int(blk[0])
        s = abs(d).bit_length()
        put(*dct[s])
        if s:
            put(d if d >= 0 else (d - 1) & ((1 << s) - 1), s)
        r = 0
        for k in range(1, 64):
            a = int(blk[k])
            if a == 0:
                r += 1
                continue
            while r > 15:
                put(*act[0xf0])
                r -= 16
            s = abs(a).bit_length()
            put(*act[r << 4 | s])
            put(a if a >= 0 else (a - 1) & ((1 << s) - 1), s)
            r = 0
        if r:
            put(*act[0])
        sizes.append(total[0] - before)
    if cnt:
        put((1 << (8 - cnt)) - 1, 8 - cnt)
    return (bytes(out), sizes) if want_bits else bytes(out)


def header(h, w, quality=75, subsampling='4:2:0', grey=False):
    """everything before the scan: SOI, APP0, DQT, SOF0, DHT, SOS"""
    hs, vs = (1, 1) if grey else SAMPLINGS[subsampling]
    n = 1 if grey else 3
    o = bytearray(b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for i, base in enumerate([QUANT_LUMA] if grey else [QUANT_LUMA, QUANT_CHROMA]):
        q = quant_table(base, quality)
        o += b'\xff\xdb\x00\x43' + bytes([i]) + bytes(q[z] for z in ZIGZAG)
    o += b'\xff\xc0' + (8 + 3 * n).to_bytes(2, 'big') + b'\x08' + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([n])
    for ci in range(n):
        o += bytes([ci + 1, (hs << 4 | vs) if ci == 0 else 0x11, 0 if ci == 0 else 1])
    tables = [(0, 0, DC_LUMA), (1, 0, AC_LUMA)] + ([] if grey else [(0, 1, DC_CHROMA), (1, 1, AC_CHROMA)])
    for cls, idx, t in tables:
        o += b'\xff\xc4' + (19 + len(t[1])).to_bytes(2, 'big') + bytes([cls << 4 | idx]) + bytes(t[0]) + bytes(t[1])
    o += b'\xff\xda' + (6 + 2 * n).to_bytes(2, 'big') + bytes([n])
    for ci in range(n):
        o += bytes([ci + 1, 0 if ci == 0 else 0x11])
    return bytes(o + b'\x00\x3f\x00')


def encode(pic, quality=75, subsampling='4:2:0'):
    pic = np.asarray(pic)
    grey = pic.ndim == 2
    b = blocks(pic, quality, subsampling)
    return header(pic.shape[0], pic.shape[1], quality, subsampling, grey) + scan(b, block_components(len(b), grey, subsampling)) + b'\xff\xd9'


def pil_encode(pic, quality=75, subsampling='4:2:0'):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(pic)).save(buf, 'JPEG', quality=quality, subsampling=PIL_SUBSAMPLING[subsampling])
    return buf.getvalue()


# ---- the pictures of the tests ---------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (2, 2), (3, 5), (8, 8), (15, 15), (16, 16), (17, 16), (16, 17), (9, 23), (31, 3), (7, 25), (25, 7), (8, 40), (40, 8), (24, 50),
         (33, 40), (48, 64), (67, 101))


def picture(kind, h, w, grey=False, seed=0):
    """'smooth', 'noise', 'flat', 'pixel_checker' (0 / 255 per pixel), 'block_checker' (0 / 255 per 8 x 8 block)"""
    rng = np.random.default_rng(seed * 7919 + h * 131 + w)
    shape = (h, w) if grey else (h, w, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == 'noise':
        a = rng.integers(0, 256, shape)
    elif kind == 'flat':
        a = np.full(shape, int(rng.integers(0, 256)))
    elif kind == 'smooth':
        a = 128 + 100 * np.sin(xx / 7.0 + rng.random()) * np.cos(yy / 5.0)
        a = a if grey else np.stack([a, a * 0.5 + 60, 255 - a], 2)
    elif kind in ('pixel_checker', 'block_checker'):
        k = 1 if kind == 'pixel_checker' else 8
        a = (((yy // k) + (xx // k)) % 2) * 255
        a = a if grey else np.stack([a, a, a], 2)
    else:
        raise ValueError(kind)
    return np.clip(a, 0, 255).astype(np.uint8)
