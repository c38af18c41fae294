"""PNG files decoded on the device (csrc/png_decode.hip, csrc/inflate_code.h): the counterpart of png.py.  A
batch of files goes in as compressed bytes and comes out as device tensors, bit for bit what PIL gives: (H, W, 3) uint8 BGR as
data.im_worker.load_bgr, or (H, W) uint8 palette / grey indices as Image.getdata() (the VOC segmentation maps).

    inflate_streams(buffers, sizes)   zlib streams (RFC 1950) inflated on the device: any stream within the limits, not only PNG data
    parse_png(data)                   the header, the palette and the IDAT bytes of one file -- or {'fallback': reason}
    decode_png(sources, mode)         paths or bytes -> device tensors; what the device does not decode comes through PIL
    stats()                           how many images were decoded on the device, and the fallbacks by reason

The host's share: the chunk walk and every chunk's CRC-32 (zlib.crc32), one upload, one read-back of the lengths and statuses."""
import ctypes
import io
import struct
import threading
import time
import zlib

import numpy as np

__all__ = ['inflate_streams', 'inflate_limits', 'parse_png', 'decode_png', 'stats', 'reset_stats', 'is_png_path', 'STATUS_BITS']

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
IMG_FIELDS = 8
TAB_FIELDS = 4
MAX_SIDE = 1 << 20
# status bits of csrc/inflate_code.h, then those of csrc/png_decode.hip
STATUS_BITS = ((1, 'zlib_header'), (2, 'block_type'), (4, 'stored_length'), (8, 'code_lengths'), (16, 'symbol'), (32, 'distance'),
               (64, 'input_end'), (128, 'capacity'), (256, 'adler'), (512, 'trailing'), (1024, 'filter_type'), (2048, 'raw_length'))
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}

_LIMITS = []
_STATS = {}
_STATS_LOCK = threading.Lock()


def inflate_limits():
    """sn_inflate_limits -> dict: max_streams, max_bytes (of a stream and of its output), lds (bytes per wave), window, lanes, flush"""
    if not _LIMITS:
        from ._lib import lib
        out = (ctypes.c_int32 * 6)()
        lib().call('sn_inflate_limits', out)
        _LIMITS.append(dict(zip(('max_streams', 'max_bytes', 'lds', 'window', 'lanes', 'flush'), (int(v) for v in out))))
    return _LIMITS[0]


def stats():
    """{'device': images decoded on the device, 'fallback': {reason: images that took PIL}}"""
    with _STATS_LOCK:
        return {'device': _STATS.get('device', 0), 'fallback': {k: v for k, v in _STATS.items() if k != 'device'}}


def reset_stats():
    with _STATS_LOCK:
        _STATS.clear()


def _count(key, n=1):
    with _STATS_LOCK:
        _STATS[key] = _STATS.get(key, 0) + n


def is_png_path(image):
    return isinstance(image, str) and image.lower().endswith('.png')


def _fallback(reason):
    return {'fallback': reason}


def _lap(timing, key, t0, sync=True):
    if timing is None:
        return t0
    if sync:
        import torch
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    timing[key] = timing.get(key, 0.0) + t1 - t0
    return t1


def _align(n, a=64):
    return (int(n) + a - 1) // a * a


# ---- inflate ---------------------------------------------------------------------------------------------------------------------
def inflate_streams(buffers, sizes, offsets=None, timing=None):
    """buffers: a list of zlib streams (bytes-likes / uint8 arrays), or (with `offsets`, (S+1) int64 on the host) one uint8 device
    tensor or array holding S streams back to back; sizes: the capacity of each output in bytes
    -> (outputs, lengths, status): S uint8 device tensors (views of one buffer, each as long as its stream inflated to, never longer
    than its capacity), the lengths (S) int64 and the status words (S) int32 on the host -- 0, or one of STATUS_BITS."""
    import torch
    from . import hip
    dev = hip.require_gpu()
    lim = inflate_limits()
    if offsets is None:
        arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8).reshape(-1) for b in buffers]
        offsets = np.concatenate([[0], np.cumsum([a.size for a in arrs])]).astype(np.int64)
        flat = np.concatenate(arrs) if len(arrs) and offsets[-1] else np.zeros(0, np.uint8)
        data = hip.dev(flat) if flat.size else torch.empty((0,), dtype=torch.uint8, device=dev)
    else:
        data = hip.dev(buffers).reshape(-1)
        if data.dtype != torch.uint8:
            raise ValueError('inflate_streams: uint8 data required, got %s' % data.dtype)
        offsets = np.ascontiguousarray(offsets, np.int64)
        if offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != data.numel():
            raise ValueError('inflate_streams: the offsets must ascend from 0 to the %d bytes of the data' % data.numel())
    S = len(offsets) - 1
    caps = np.ascontiguousarray(sizes, np.int64).reshape(-1)
    if S < 1 or S > lim['max_streams'] or caps.size != S:
        raise ValueError('inflate_streams: %d streams and %d sizes, 1 .. %d streams per call' % (S, caps.size, lim['max_streams']))
    if (caps < 0).any() or caps.max() > lim['max_bytes'] or np.diff(offsets).max() > lim['max_bytes']:
        raise ValueError('inflate_streams: a stream or a capacity is above %d bytes (or negative)' % lim['max_bytes'])
    t0 = time.perf_counter()
    tab = np.zeros((S, TAB_FIELDS), np.int64)
    tab[:, 0], tab[:, 1] = offsets[:-1], np.diff(offsets)
    aligned = (caps + 15) // 16 * 16
    tab[:, 2] = np.concatenate([[0], np.cumsum(aligned)[:-1]])
    tab[:, 3] = caps
    out_total = int(aligned.sum())
    out = torch.empty((max(out_total, 1),), dtype=torch.uint8, device=dev)
    meta = torch.zeros((S, 2), dtype=torch.int32, device=dev)
    hip.call('sn_inflate', data if data.numel() else None, int(offsets[-1]), hip.dev(tab), tab, S, out, out_total, meta, hip.stream())
    t0 = _lap(timing, 'inflate_s', t0)
    h_meta = meta.cpu().numpy()
    _lap(timing, 'status_s', t0)
    lengths = h_meta[:, 0].astype(np.int64)
    if (lengths > caps).any():
        raise RuntimeError('inflate_streams: a stream came out longer than its capacity')
    return [out[int(o):int(o) + int(n)] for o, n in zip(tab[:, 2], lengths)], lengths, h_meta[:, 1].copy()


# ---- the container ---------------------------------------------------------------------------------------------------------------
def parse_png(data, mode='bgr'):
    """data: the bytes of a file -> dict
         W, H, depth, ctype (the colour type), channels, row (bytes per row), bpp (the filters' pixel distance in bytes), raw_len =
         H * (row + 1), palette (256, 3) uint8 zero-padded, plen (its entries in the file), idat (the IDAT bytes joined: one zlib stream)
       or {'fallback': reason} for what the device does not decode: bad_header (signature, IHDR, chunk order, PLTE), truncated,
       bad_crc (any chunk), interlaced, gray16, apng, no_idat, too_large, and in index mode not_indexed."""
    d = bytes(data) if not isinstance(data, bytes) else data
    n = len(d)
    if n < 8:
        return _fallback('truncated' if d == PNG_SIGNATURE[:n] else 'bad_header')
    if d[:8] != PNG_SIGNATURE:
        return _fallback('bad_header')
    pos = 8
    ihdr = None
    palette, plen = np.zeros((256, 3), np.uint8), 0
    idat, idat_done, apng, ended, have_plte = [], False, False, False, False
    while not ended:
        if pos + 12 > n:
            return _fallback('truncated')
        L, kind = struct.unpack('>I4s', d[pos:pos + 8])
        if L > 0x7fffffff:
            return _fallback('bad_header')
        if pos + 12 + L > n:
            return _fallback('truncated')
        body = d[pos + 8:pos + 8 + L]
        if zlib.crc32(body, zlib.crc32(kind)) & 0xffffffff != struct.unpack('>I', d[pos + 8 + L:pos + 12 + L])[0]:
            return _fallback('bad_crc')
        pos += 12 + L
        if ihdr is None:
            if kind != b'IHDR' or L != 13:
                return _fallback('bad_header')
            ihdr = struct.unpack('>IIBBBBB', body)
            continue
        if kind == b'IHDR':
            return _fallback('bad_header')
        if kind == b'IDAT':
            if idat_done:
                return _fallback('bad_header')          # the IDAT chunks must be consecutive
            idat.append(body)
            continue
        if idat:
            idat_done = True
        if kind == b'PLTE':
            if have_plte or idat or L % 3 or L > 768 or L == 0:
                return _fallback('bad_header')
            have_plte = True
            plen = L // 3
            palette[:plen] = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b'acTL':
            apng = True
        elif kind == b'IEND':
            ended = True
    W, H, depth, ctype, comp, filt, lace = ihdr
    if W < 1 or H < 1 or W > 0x7fffffff or H > 0x7fffffff or ctype not in CHANNELS or depth not in DEPTHS[ctype] or comp != 0 or filt != 0 or lace > 1:
        return _fallback('bad_header')
    if ctype == 3 and not have_plte:
        return _fallback('bad_header')
    if apng:
        return _fallback('apng')
    if lace:
        return _fallback('interlaced')
    if depth == 16 and ctype in (0, 4):
        return _fallback('gray16')
    if not idat:
        return _fallback('no_idat')
    if mode == 'index' and ctype not in (0, 3):
        return _fallback('not_indexed')
    ch = CHANNELS[ctype]
    row = (W * ch * depth + 7) // 8
    raw_len = H * (row + 1)
    z = idat[0] if len(idat) == 1 else b''.join(idat)
    lim = inflate_limits() if _LIMITS else {'max_bytes': 1 << 30}
    if W > MAX_SIDE or H > MAX_SIDE or W * H >= 1 << 29 or raw_len > lim['max_bytes'] or len(z) > lim['max_bytes']:
        return _fallback('too_large')
    return dict(W=W, H=H, depth=depth, ctype=ctype, channels=ch, row=row, bpp=max(1, ch * depth // 8), raw_len=raw_len, palette=palette,
                plen=plen if ctype == 3 else 0, idat=z)


def _read(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, 'rb') as fh:
        return fh.read()


def _host_decode(src, mode):
    """what the parent path gives: load_bgr's pixels, or in index mode what the reference's parse_inst reads"""
    where = io.BytesIO(src) if isinstance(src, (bytes, bytearray, memoryview)) else src
    if mode == 'bgr':
        from .data.im_worker import load_bgr
        return load_bgr(where)
    from PIL import Image
    im = Image.open(where)
    return np.array(im.getdata(), np.uint8).reshape(im.size[1], im.size[0])


def _status_reason(word):
    for bit, name in STATUS_BITS:
        if word & bit:
            return 'damaged_' + name
    return 'damaged'


def decode_png(sources, mode='bgr', timing=None):
    """sources: paths or bytes; a batch may mix sizes, depths and colour types -> a list of uint8 device tensors in order, every tensor
    owning its storage: mode 'bgr' (H, W, 3) as load_bgr gives them, mode 'index' (H, W) palette indices / grey samples as
    np.array(Image.getdata(), np.uint8) gives them for P and L images.  What the device does not decode (parse_png's fallbacks,
    streams the kernels flag) comes through PIL, which may raise as it does today.
    timing: a dict that collects the stages in seconds, each closed by a synchronise."""
    from . import hip
    if mode not in ('bgr', 'index'):
        raise ValueError("decode_png: mode %r: 'bgr' or 'index' required" % (mode,))
    dev = hip.require_gpu()
    sources = list(sources)
    out = [None] * len(sources)
    t0 = time.perf_counter()
    blobs = [_read(s) for s in sources]
    t0 = _lap(timing, 'read_s', t0, sync=False)
    inflate_limits()
    heads = [parse_png(b, mode) for b in blobs]
    t0 = _lap(timing, 'parse_s', t0, sync=False)
    lim = inflate_limits()
    todo = [i for i, h in enumerate(heads) if 'fallback' not in h]
    start = 0
    while start < len(todo):          # batches whose pooled sizes stay below 2^31 bytes; one batch for any ordinary call
        stop, nbytes = start, 0
        while stop < len(todo) and stop - start < lim['max_streams']:
            h = heads[todo[stop]]
            b = len(h['idat']) + h['raw_len'] + h['W'] * h['H'] * 3
            if stop > start and nbytes + b > (1 << 31):
                break
            nbytes, stop = nbytes + b, stop + 1
        _decode_batch(todo[start:stop], heads, out, mode, timing, dev)
        start = stop
    t0 = time.perf_counter()
    for i, h in enumerate(heads):
        if out[i] is None:
            _count(h.get('fallback') or h['flagged'])
            out[i] = hip.dev(_host_decode(sources[i], mode))
    _lap(timing, 'fallback_s', t0)
    return out


def _decode_batch(idx, heads, out, mode, timing, dev):
    import torch
    from . import hip
    t0 = time.perf_counter()
    I = len(idx)
    img = np.zeros((I, IMG_FIELDS), np.int32)
    raw_off = np.zeros((I,), np.int64)
    tab = np.zeros((I, TAB_FIELDS), np.int64)
    pal = np.zeros((I, 768), np.uint8)
    in0 = raw0 = 0
    for j, i in enumerate(idx):
        h = heads[i]
        img[j] = (h['W'], h['H'], h['depth'], h['ctype'], h['row'], h['bpp'], h['plen'], 0)
        raw_off[j] = raw0
        tab[j] = (in0, len(h['idat']), raw0, h['raw_len'])
        pal[j] = h['palette'].reshape(-1)
        in0 += _align(len(h['idat']))
        raw0 += _align(h['raw_len'])
    total_in, raw_total = in0, raw0
    shape = (lambda j: (int(img[j, 1]), int(img[j, 0]), 3)) if mode == 'bgr' else (lambda j: (int(img[j, 1]), int(img[j, 0])))
    tensors = [torch.empty(shape(j), dtype=torch.uint8, device=dev) for j in range(I)]
    ptrs = np.array([t.data_ptr() for t in tensors], np.uint64)
    # one upload: the tables, then the streams
    parts = [img.view(np.uint8).reshape(-1), raw_off.view(np.uint8), tab.view(np.uint8).reshape(-1), pal.reshape(-1), ptrs.view(np.uint8)]
    offs, at = [], 0
    for p in parts:
        offs.append(at)
        at += _align(p.size)
    data_off = at
    host = np.zeros(at + total_in, np.uint8)
    for p, o in zip(parts, offs):
        host[o:o + p.size] = p
    for j, i in enumerate(idx):
        o = data_off + int(tab[j, 0])
        host[o:o + int(tab[j, 1])] = np.frombuffer(heads[i]['idat'], np.uint8)
    t0 = _lap(timing, 'tables_s', t0, sync=False)
    blob = torch.from_numpy(host).to(dev)
    d_img, d_raw_off, d_tab, d_pal, d_ptr = (blob[o:] for o in offs)
    d_data = blob[data_off:]
    raw = torch.empty((raw_total,), dtype=torch.uint8, device=dev)
    meta = torch.zeros((I, 2), dtype=torch.int32, device=dev)
    t0 = _lap(timing, 'upload_s', t0)
    st = hip.stream()
    hip.call('sn_inflate', d_data, total_in, d_tab, tab, I, raw, raw_total, meta, st)
    t0 = _lap(timing, 'inflate_s', t0)
    hip.call('sn_png_unfilter', raw, raw_total, d_img, img, d_raw_off, raw_off, I, meta, st)
    t0 = _lap(timing, 'unfilter_s', t0)
    hip.call('sn_png_expand', raw, raw_total, d_img, img, d_raw_off, raw_off, I, d_pal, d_ptr, meta, 0 if mode == 'bgr' else 1, st)
    t0 = _lap(timing, 'expand_s', t0)
    h_meta = meta.cpu().numpy()          # the one read-back: lengths and statuses
    _lap(timing, 'status_s', t0)
    good = 0
    for j, i in enumerate(idx):
        if h_meta[j, 1] == 0:
            out[i] = tensors[j]
            good += 1
        else:
            heads[i]['flagged'] = _status_reason(int(h_meta[j, 1]))
    _count('device', good)
