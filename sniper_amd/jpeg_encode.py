"""Baseline JPEG files from pictures on the device (csrc/jpeg_encode.hip, csrc/jpeg_enc_code.h): colour
conversion, downsampling, forward DCT, quantisation, Huffman coding and byte stuffing.  A file is byte for byte the file PIL
(libjpeg-turbo) writes for Image.save(path, quality=q, subsampling=s) -- with no arguments quality 75, 4:2:0 -- so who encodes
changes no output.  A rendered batch (visualization.render_lists of device tensors) is encoded without its raw bytes leaving HBM:
what comes to the host is one read-back of the scan lengths and the compressed bytes.

    jpeg_quant_tables(quality)                          the scaled Annex K tables (host)
    jpeg_header(h, w, quality, subsampling, grey)       everything before the scan (host)
    jpeg_coefficients(pictures, quality, subsampling)   the quantised blocks in scan order, on the device
    encode_jpeg(pictures, quality, subsampling)         the files' bytes
    write_jpeg(paths, pictures, ...)                    the files
    stats()                                             files and bytes encoded on the device

The host's share: the headers, joining header, scan and EOI, the file writes.  Not encoded here, and refused with ValueError before
anything is launched: optimised Huffman tables, progressive, restart markers, EXIF / ICC / dpi, CMYK, other samplings,
quality='keep' and presets."""
import ctypes
import threading
import time

import numpy as np

__all__ = ['jpeg_quant_tables', 'jpeg_header', 'jpeg_coefficients', 'encode_jpeg', 'write_jpeg', 'stats', 'reset_stats', 'jpeg_enc_limits',
           'SUBSAMPLINGS']

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# T.81 annex K.1 (natural order) and K.3 (counts of the code lengths 1 .. 16, then the values)
_QUANT = ((16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
          (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
_DC_BITS = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0))
_AC_BITS = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77))
_AC_VALS = (bytes.fromhex('01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a'
                          '434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa'
                          'b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'),
            bytes.fromhex('000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a'
                          '434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa'
                          'b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa'))
# subsampling -> the code of the C ABI (PIL's own numbering)
SUBSAMPLINGS = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}
_LUMA_FACTORS = {0: (1, 1), 1: (2, 1), 2: (2, 2)}

_LIMITS = []
_STATS = {}
_STATS_LOCK = threading.Lock()


def jpeg_enc_limits():
    """sn_jpeg_enc_limits -> dict: threads, max_pictures, max_blocks (per call), raw_bytes_per_block, chunk, blocks_lds, code_lds,
    stuffed_per_raw"""
    if not _LIMITS:
        from ._lib import lib
        out = (ctypes.c_int32 * 8)()
        lib().call('sn_jpeg_enc_limits', out)
        _LIMITS.append(dict(zip(('threads', 'max_pictures', 'max_blocks', 'raw_bytes_per_block', 'chunk', 'blocks_lds', 'code_lds', 'stuffed_per_raw'),
                                (int(v) for v in out))))
    return _LIMITS[0]


def stats():
    """{'files': files encoded on the device, 'bytes': their bytes}"""
    with _STATS_LOCK:
        return {'files': _STATS.get('files', 0), 'bytes': _STATS.get('bytes', 0)}


def reset_stats():
    with _STATS_LOCK:
        _STATS.clear()


def _check(quality, subsampling):
    if isinstance(quality, bool) or not isinstance(quality, (int, np.integer)) or not 1 <= int(quality) <= 100:
        raise ValueError('jpeg: quality=%r: an integer 1 .. 100 (presets and \'keep\' are not encoded here)' % (quality,))
    if subsampling not in SUBSAMPLINGS:
        raise ValueError("jpeg: subsampling=%r: '4:2:0', '4:2:2' or '4:4:4'" % (subsampling,))
    return int(quality), SUBSAMPLINGS[subsampling]


def jpeg_quant_tables(quality=75):
    """-> (2, 64) int: the luminance and the chrominance table in natural order: clamp((base * s + 50) // 100, 1, 255) with
    s = 5000 // quality below 50, else 200 - 2 * quality"""
    quality, _ = _check(quality, '4:2:0')
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(_QUANT, np.int64) * s + 50) // 100, 1, 255)


def jpeg_header(h, w, quality=75, subsampling='4:2:0', grey=False):
    """SOI, APP0 (JFIF 1.01, no density unit, 1 x 1), one DQT per table, SOF0, the DHT segments (DC 0, AC 0, DC 1, AC 1), SOS:
    everything before the scan, as libjpeg writes it"""
    quality, code = _check(quality, subsampling)
    h, w = int(h), int(w)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError('jpeg: a picture of %d x %d: 1 <= h, w <= 65535' % (h, w))
    hs, vs = (1, 1) if grey else _LUMA_FACTORS[code]
    n = 1 if grey else 3
    tabs = jpeg_quant_tables(quality)
    o = [b'\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00']
    for t in range(1 if grey else 2):
        o.append(b'\xff\xdb\x00\x43' + bytes([t]) + bytes(int(tabs[t][z]) for z in ZIGZAG))
    o.append(b'\xff\xc0' + (8 + 3 * n).to_bytes(2, 'big') + b'\x08' + h.to_bytes(2, 'big') + w.to_bytes(2, 'big') + bytes([n]))
    for c in range(n):
        o.append(bytes([c + 1, (hs << 4 | vs) if c == 0 else 0x11, 0 if c == 0 else 1]))
    for t in range(1 if grey else 2):
        o.append(b'\xff\xc4\x00\x1f' + bytes([t]) + bytes(_DC_BITS[t]) + bytes(range(12)))
        o.append(b'\xff\xc4\x00\xb5' + bytes([0x10 | t]) + bytes(_AC_BITS[t]) + _AC_VALS[t])
    o.append(b'\xff\xda' + (6 + 2 * n).to_bytes(2, 'big') + bytes([n]))
    for c in range(n):
        o.append(bytes([c + 1, 0 if c == 0 else 0x11]))
    o.append(b'\x00\x3f\x00')
    return b''.join(o)


def _lap(timing, key, t0, sync=True):
    if timing is None:
        return t0
    if sync:
        import torch
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    timing[key] = timing.get(key, 0.0) + t1 - t0
    return t1


def _is_device(p):
    import torch
    return isinstance(p, torch.Tensor) and p.is_cuda


def _kind(p):
    """1 (grey) or 3 (RGB); anything else is refused"""
    shape = tuple(int(v) for v in p.shape)
    ok = str(p.dtype).endswith('uint8') and (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3))
    if not ok or not (1 <= shape[0] <= 65535 and 1 <= shape[1] <= 65535):
        raise ValueError('jpeg: (h, w, 3) or (h, w) uint8 pictures with 1 <= h, w <= 65535 required, got %s %s' % (shape, p.dtype))
    return 1 if len(shape) == 2 else 3


def _blocks_of(h, w, ncomp, code):
    hs, vs = _LUMA_FACTORS[code] if ncomp == 3 else (1, 1)
    return -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + ncomp - 1)


class _Batch(object):
    """pictures of one kind, packed for one call: the pixels on the device, the sizes and offsets on both sides"""

    def __init__(self, pictures, ncomp, code):
        import torch
        from . import hip
        self.ncomp, self.code, self.I = ncomp, code, len(pictures)
        self.hw = np.array([[int(p.shape[0]), int(p.shape[1])] for p in pictures], np.int32).reshape(-1, 2)
        hw64 = self.hw.astype(np.int64)
        self.pix_off = np.concatenate([[0], np.cumsum(hw64[:, 0] * hw64[:, 1])]).astype(np.int64)
        self.blk_off = np.concatenate([[0], np.cumsum([_blocks_of(h, w, ncomp, code) for h, w in hw64])]).astype(np.int64)
        self.n_blocks = int(self.blk_off[-1])
        if any(_is_device(p) for p in pictures):
            # device tensors do not come to the host: the others are uploaded one by one, then a device-to-device copy
            flat = [p.contiguous().reshape(-1) if _is_device(p) else hip.dev(np.ascontiguousarray(p, np.uint8).reshape(-1)) for p in pictures]
            self.pix = flat[0] if self.I == 1 else torch.cat(flat)
        else:
            self.pix = hip.dev(np.concatenate([np.ascontiguousarray(p, np.uint8).reshape(-1) for p in pictures]))
        # one upload for the three small tables
        table = np.concatenate([self.pix_off, self.blk_off, self.hw.reshape(-1).astype(np.int64)])
        d = hip.dev(table)
        self.d_pix_off, self.d_blk_off = d[:self.I + 1], d[self.I + 1:2 * self.I + 2]
        self.d_hw = d[2 * self.I + 2:].to(torch.int32)


def _split(pictures, code):
    """-> [(ncomp, [indices])]: calls of one kind each, inside the limits of a call"""
    lim = jpeg_enc_limits()
    calls = []
    for ncomp in (3, 1):
        cur, blocks = [], 0
        for i, p in enumerate(pictures):
            if _kind(p) != ncomp:
                continue
            nb = _blocks_of(int(p.shape[0]), int(p.shape[1]), ncomp, code)
            if nb > lim['max_blocks']:
                raise ValueError('jpeg: a picture of %d x %d has %d blocks; a call takes %d' % (int(p.shape[0]), int(p.shape[1]), nb, lim['max_blocks']))
            if cur and (blocks + nb > lim['max_blocks'] or len(cur) >= lim['max_pictures']):
                calls.append((ncomp, cur))
                cur, blocks = [], 0
            cur.append(i)
            blocks += nb
        if cur:
            calls.append((ncomp, cur))
    return calls


def _coefficients(batch, quality):
    import torch
    from . import hip
    coef = torch.empty((batch.n_blocks, 64), dtype=torch.int16, device=batch.pix.device)
    hip.call('sn_jpeg_enc_blocks', batch.pix, int(batch.pix_off[-1]), batch.d_hw, batch.hw, batch.d_pix_off, batch.pix_off, batch.d_blk_off,
             batch.blk_off, batch.I, batch.n_blocks, batch.ncomp, batch.code, quality, coef, hip.stream())
    return coef


def jpeg_coefficients(pictures, quality=75, subsampling='4:2:0'):
    """pictures of ONE kind ((h, w, 3) RGB or (h, w) grey, uint8, numpy arrays or device tensors, sizes may differ) -> (coef, offsets):
    coef (n_blocks, 64) int16 on the device -- every block of every scan in scan order (MCUs in raster order; inside an MCU the luma
    blocks row-major, then Cb, then Cr), zig-zag order inside a block, quantised, the DC not yet differenced, the dummy blocks of edge
    MCUs resolved -- and the (I+1) block offsets of the pictures on the host.  The stage before coding, as png_filter is for PNG."""
    quality, code = _check(quality, subsampling)
    pictures = list(pictures)
    if not pictures:
        raise ValueError('jpeg: no pictures')
    kinds = set(_kind(p) for p in pictures)
    if len(kinds) != 1:
        raise ValueError('jpeg_coefficients: grey and RGB pictures in one call')
    calls = _split(pictures, code)
    if len(calls) != 1:
        raise ValueError('jpeg_coefficients: more blocks than one call takes (%d)' % jpeg_enc_limits()['max_blocks'])
    from . import hip
    hip.require_gpu()
    batch = _Batch(pictures, kinds.pop(), code)
    return _coefficients(batch, quality), batch.blk_off


def _encode_call(pictures, ncomp, quality, code, timing, guard=0):
    """-> (host uint8 array of the scans back to back, (I+1) offsets); guard: bytes of a pattern behind the capacity (tests)"""
    import torch
    from . import hip
    dev = hip.require_gpu()
    lim = jpeg_enc_limits()
    t0 = time.perf_counter()
    batch = _Batch(pictures, ncomp, code)
    I, N, chunk = batch.I, batch.n_blocks, lim['chunk']
    t0 = _lap(timing, 'upload_s', t0)
    st = hip.stream()
    coef = _coefficients(batch, quality)
    t0 = _lap(timing, 'blocks_s', t0)
    bits = torch.empty((N,), dtype=torch.int32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    hip.call('sn_jpeg_enc_size', coef, batch.d_hw, batch.hw, batch.d_blk_off, batch.blk_off, I, N, ncomp, code, bits, status, st)
    t0 = _lap(timing, 'size_s', t0)
    # the capacities from the derived bound (no read-back of sizes): a block's code is at most 22 + 63 * 26 bits = 208 bytes, a
    # picture's last byte is filled, its raw stream starts on a chunk; stuffing at most doubles a byte
    per_pic = -(-(np.diff(batch.blk_off) * lim['raw_bytes_per_block'] + 1) // chunk)
    n_chunks = int(per_pic.sum())
    raw_capacity = n_chunks * chunk
    capacity = lim['stuffed_per_raw'] * raw_capacity
    ends = torch.cumsum(bits, 0, dtype=torch.int64)
    bit_excl = ends - bits
    pic_first_bit = bit_excl[batch.d_blk_off[:-1]]
    pic_bits = ends[batch.d_blk_off[1:] - 1] - pic_first_bit
    raw_len = (pic_bits + 7) >> 3
    chunk_off = torch.zeros((I + 1,), dtype=torch.int64, device=dev)
    torch.cumsum((raw_len + (chunk - 1)) // chunk, 0, out=chunk_off[1:])
    raw = torch.zeros((raw_capacity // 4,), dtype=torch.int32, device=dev)
    t0 = _lap(timing, 'scan_s', t0)
    hip.call('sn_jpeg_enc_write', coef, batch.d_hw, batch.hw, batch.d_blk_off, batch.blk_off, I, N, ncomp, code, bit_excl, pic_first_bit,
             chunk_off, raw, raw_capacity, status, st)
    t0 = _lap(timing, 'write_s', t0)
    cnt = torch.empty((n_chunks,), dtype=torch.int32, device=dev)
    out = torch.empty((capacity + guard,), dtype=torch.uint8, device=dev)
    if guard:
        out[capacity:] = 0xa5
    t0 = _lap(timing, 'alloc_s', t0)
    hip.call('sn_jpeg_enc_stuff', raw, raw_capacity, chunk_off, raw_len, I, n_chunks, 1, cnt, None, None, 0, st)
    t0 = _lap(timing, 'count_s', t0)
    out_end = torch.cumsum(cnt, 0, dtype=torch.int64)
    out_pos = out_end - cnt
    t0 = _lap(timing, 'stuff_scan_s', t0)
    hip.call('sn_jpeg_enc_stuff', raw, raw_capacity, chunk_off, raw_len, I, n_chunks, 2, None, out_pos, out, capacity, st)
    # picture i's scan starts where its first chunk does; the last entry is the total; the status word rides along
    out_off = torch.cat([out_pos, out_end[-1:]])[torch.clamp(chunk_off, max=n_chunks)]
    lengths = torch.cat([out_off, status.long()])
    t0 = _lap(timing, 'stuff_s', t0)
    h_len = lengths.cpu().numpy()          # the one read-back before the download: I + 1 offsets and the status
    t0 = _lap(timing, 'lengths_s', t0)
    h_off, h_status = h_len[:-1], int(h_len[-1])
    n_out = int(h_off[-1])
    if h_status or n_out > capacity or h_off[0] != 0 or (np.diff(h_off) < 1).any():
        raise RuntimeError('encode_jpeg: status %d, %d bytes for a capacity of %d' % (h_status, n_out, capacity))
    host = out[:n_out].cpu().numpy()
    if guard and not bool((out[capacity:] == 0xa5).all()):
        raise RuntimeError('encode_jpeg: the bytes behind the capacity were written')
    _lap(timing, 'download_s', t0)
    return host, h_off


def encode_jpeg(pictures, quality=75, subsampling='4:2:0', timing=None, _guard=0):
    """pictures: (h, w, 3) uint8 RGB or (h, w) uint8 grey, numpy arrays or device tensors, mixed, sizes may differ -> the bytes of one
    baseline JFIF file per picture: the file PIL writes at the same quality (1 .. 100) and subsampling ('4:2:0', '4:2:2', '4:4:4';
    ignored for grey).  timing: a dict that collects the stages in seconds, each closed by a synchronise."""
    quality, code = _check(quality, subsampling)
    pictures = list(pictures)
    if not pictures:
        raise ValueError('jpeg: no pictures')
    files = [None] * len(pictures)
    headers = {}          # (pictures of one size share their header)
    for ncomp, idx in _split(pictures, code):          # (every picture is checked before the first launch)
        host, off = _encode_call([pictures[i] for i in idx], ncomp, quality, code, timing, _guard)
        t0 = time.perf_counter()
        for j, i in enumerate(idx):
            key = (int(pictures[i].shape[0]), int(pictures[i].shape[1]), ncomp)
            if key not in headers:
                headers[key] = jpeg_header(key[0], key[1], quality, subsampling, ncomp == 1)
            files[i] = b''.join((headers[key], memoryview(host[off[j]:off[j + 1]]), b'\xff\xd9'))
        _lap(timing, 'join_s', t0, sync=False)
    with _STATS_LOCK:
        _STATS['files'] = _STATS.get('files', 0) + len(files)
        _STATS['bytes'] = _STATS.get('bytes', 0) + sum(len(f) for f in files)
    return files


def write_jpeg(paths, pictures, quality=75, subsampling='4:2:0', timing=None):
    """encode_jpeg, then one file per picture"""
    paths, pictures = list(paths), list(pictures)
    if len(paths) != len(pictures):
        raise ValueError('write_jpeg: %d paths for %d pictures' % (len(paths), len(pictures)))
    files = encode_jpeg(pictures, quality, subsampling, timing)
    t0 = time.perf_counter()
    for path, data in zip(paths, files):
        with open(path, 'wb') as fh:
            fh.write(data)
    _lap(timing, 'file_s', t0, sync=False)
    return paths
