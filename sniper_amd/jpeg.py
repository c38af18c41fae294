"""Baseline JPEG files decoded on the device (csrc/jpeg_decode.hip, csrc/jpeg_entropy.h): a batch of files goes in
as compressed bytes and comes out as (H, W, 3) uint8 BGR device tensors, bit for bit what data.im_worker.load_bgr gives (PIL over
libjpeg: slow-integer IDCT, fancy upsampling).

    parse_jpeg(data)                  the header, the tables and the segments of one file -- or {'fallback': reason}
    decode_jpeg(sources)              paths or bytes -> device tensors; what the device does not decode comes through load_bgr
    stats()                           how many images were decoded on the device, and the fallbacks by reason

The host's share: finding the markers (one numpy pass over the bytes), the tables, one upload, one read-back of the statuses."""
import ctypes
import io
import threading
import time

import numpy as np

__all__ = ['parse_jpeg', 'decode_jpeg', 'stats', 'reset_stats', 'jpeg_limits', 'is_jpeg_path']

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                   49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DHT_BYTES = 16 + 256
IMG_FIELDS = 16
MAX_SEGMENT_SUBS = 16384      # csrc/jpeg_decode.hip: kMaxSegmentSubs
SEG_FIELDS = 8
# status bits of csrc/jpeg_entropy.h
STATUS_BITS = ((1, 'bad_code'), (2, 'bad_run'), (4, 'overrun'), (8, 'blocks'), (16, 'bad_dc'), (32, 'range'), (64, 'bad_marker'))

_LIMITS = []
_STATS = {}
_STATS_LOCK = threading.Lock()


def jpeg_limits():
    """sn_jpeg_limits -> dict: sub (bytes of a subsequence), threads, max_images, max_bpm, huff_lds, img_fields, seg_fields, min_sub"""
    if not _LIMITS:
        from ._lib import lib
        out = (ctypes.c_int32 * 8)()
        lib().call('sn_jpeg_limits', out)
        _LIMITS.append(dict(zip(('sub', 'threads', 'max_images', 'max_bpm', 'huff_lds', 'img_fields', 'seg_fields', 'min_sub'), (int(v) for v in out))))
    return _LIMITS[0]


def stats():
    """{'device': images decoded on the device, 'fallback': {reason: images that took load_bgr}}"""
    with _STATS_LOCK:
        return {'device': _STATS.get('device', 0), 'fallback': {k: v for k, v in _STATS.items() if k != 'device'}}


def reset_stats():
    with _STATS_LOCK:
        _STATS.clear()


def _count(key, n=1):
    with _STATS_LOCK:
        _STATS[key] = _STATS.get(key, 0) + n


def is_jpeg_path(image):
    return isinstance(image, str) and image.lower().endswith(('.jpg', '.jpeg', '.jpe', '.jfif'))


def _fallback(reason):
    return {'fallback': reason}


def parse_jpeg(data):
    """data: the bytes of a file -> dict
         H, W, ncomp, hs, vs (the luma sampling; chroma is 1 x 1), mcux, mcuy, bpm (blocks per MCU), ri (MCUs per restart interval, 0:
         none), qtab (ncomp, 64) uint16 in natural order, dht (4, 272) uint8: DC 0, DC 1, AC 0, AC 1 as the DHT segments hold them,
         sel (bit 2c: DC table of component c, bit 2c + 1: its AC table), seg_first / seg_end (byte ranges of the restart intervals,
         markers excluded), scan (first byte of the entropy-coded data)
       or {'fallback': reason} for what the device does not decode."""
    d = np.frombuffer(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8)
    n = d.size
    if n < 4 or d[0] != 0xff or d[1] != 0xd8:
        return _fallback('not_jpeg')
    pos = 2
    qt = {}
    dht = np.zeros((4, DHT_BYTES), np.uint8)
    have_dht = set()
    sof = None
    ri = 0
    jfif = adobe = False
    while True:
        if pos + 4 > n:
            return _fallback('damaged_header')
        if d[pos] != 0xff:
            return _fallback('damaged_header')
        m = int(d[pos + 1])
        if m == 0xff:
            pos += 1
            continue
        if m == 0x01 or 0xd0 <= m <= 0xd8:
            pos += 2
            continue
        if m == 0xd9:
            return _fallback('no_scan')
        L = (int(d[pos + 2]) << 8) | int(d[pos + 3])
        if L < 2 or pos + 2 + L > n:
            return _fallback('damaged_header')
        body = d[pos + 4:pos + 2 + L]
        if m == 0xe0 and body.size >= 5 and bytes(body[:5]) == b'JFIF\0':
            jfif = True
        elif m == 0xee and body.size >= 12 and bytes(body[:5]) == b'Adobe':
            adobe = True
        elif m == 0xdb:
            q = 0
            while q < body.size:
                pq, tq = int(body[q]) >> 4, int(body[q]) & 15
                if pq != 0:
                    return _fallback('quant16')
                if tq > 3 or q + 65 > body.size:
                    return _fallback('damaged_header')
                qt[tq] = body[q + 1:q + 65].astype(np.uint16)
                q += 65
        elif m == 0xc4:
            q = 0
            while q < body.size:
                if q + 17 > body.size:
                    return _fallback('damaged_header')
                tc, th = int(body[q]) >> 4, int(body[q]) & 15
                cnt = int(body[q + 1:q + 17].sum())
                if tc > 1 or cnt > 256 or q + 17 + cnt > body.size:
                    return _fallback('damaged_header')
                if th > 1:
                    return _fallback('tables')
                dht[tc * 2 + th] = 0
                dht[tc * 2 + th, :16 + cnt] = body[q + 1:q + 17 + cnt]
                have_dht.add(tc * 2 + th)
                q += 17 + cnt
        elif m == 0xdd:
            if L != 4:
                return _fallback('damaged_header')
            ri = (int(body[0]) << 8) | int(body[1])
        elif m == 0xc0:
            if sof is not None or body.size < 6:
                return _fallback('damaged_header')
            sof = body
        elif m == 0xc2 or m == 0xc6 or m == 0xca or m == 0xce:
            return _fallback('progressive')
        elif 0xc9 <= m <= 0xcf and m != 0xcc:
            return _fallback('arithmetic')
        elif m in (0xc1, 0xc3, 0xc5, 0xc7, 0xcc, 0xdc):
            return _fallback('sof')
        elif m == 0xda:
            break
        pos += 2 + L
    if sof is None:
        return _fallback('damaged_header')
    if int(sof[0]) != 8:
        return _fallback('12bit')
    H, W, nc = (int(sof[1]) << 8) | int(sof[2]), (int(sof[3]) << 8) | int(sof[4]), int(sof[5])
    if H < 1 or W < 1 or sof.size < 6 + 3 * nc:
        return _fallback('damaged_header')
    if nc == 4:
        return _fallback('cmyk')
    if nc not in (1, 3):
        return _fallback('components')
    comps = [(int(sof[6 + 3 * c]), int(sof[7 + 3 * c]) >> 4, int(sof[7 + 3 * c]) & 15, int(sof[8 + 3 * c])) for c in range(nc)]
    if nc == 3:
        if adobe and not jfif:
            return _fallback('adobe')
        if not jfif and tuple(c[0] for c in comps) == (82, 71, 66):
            return _fallback('rgb')
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return _fallback('sampling')
        if hs == 2 and W <= 2:
            return _fallback('narrow_chroma')
    else:
        hs = vs = 1          # a scan of one component is not interleaved: one block per MCU whatever the header says
    # the scan header
    if body.size < 1 or int(body[0]) != nc or body.size < 1 + 2 * nc + 3:
        return _fallback('multiscan')
    sel = 0
    for c in range(nc):
        cs, tt = int(body[1 + 2 * c]), int(body[2 + 2 * c])
        if cs != comps[c][0]:
            return _fallback('multiscan')
        td, ta = tt >> 4, tt & 15
        if td > 1 or ta > 1:
            return _fallback('tables')
        if td not in have_dht or (2 + ta) not in have_dht:
            return _fallback('damaged_header')
        sel |= (td << (2 * c)) | (ta << (2 * c + 1))
    if (int(body[1 + 2 * nc]), int(body[2 + 2 * nc]), int(body[3 + 2 * nc])) != (0, 63, 0):
        return _fallback('multiscan')
    qtab = np.zeros((nc, 64), np.uint16)
    for c in range(nc):
        if comps[c][3] not in qt:
            return _fallback('damaged_header')
        qtab[c, ZIGZAG] = qt[comps[c][3]]
    scan = pos + 2 + L
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    bpm = hs * vs + (nc - 1)
    n_mcu = mcux * mcuy
    # markers inside and after the entropy-coded data: an FF that a zero does not follow
    ff = np.flatnonzero(d[scan:n - 1] == 0xff) + scan
    mk = ff[d[ff + 1] != 0]
    codes = d[mk + 1] if mk.size else np.zeros(0, np.uint8)
    if (codes == 0xff).any():
        return _fallback('fill_bytes')
    rst = (codes >= 0xd0) & (codes <= 0xd7)
    stop = np.flatnonzero(~rst)
    if stop.size:
        k = int(stop[0])
        end = int(mk[k])
        if int(codes[k]) != 0xd9:
            return _fallback('multiscan')
        mk, codes = mk[:k], codes[:k]
    else:
        end = n              # no EOI: the data runs to the end of the file (a truncated file; the kernels say so)
    n_seg = -(-n_mcu // ri) if ri else 1
    if mk.size != n_seg - 1 or (codes != (0xd0 + (np.arange(mk.size) & 7))).any():
        return _fallback('damaged_markers')
    seg_first = np.concatenate([[scan], mk + 2]).astype(np.int64)
    seg_end = np.concatenate([mk, [end]]).astype(np.int64)
    return dict(H=H, W=W, ncomp=nc, hs=hs, vs=vs, mcux=mcux, mcuy=mcuy, bpm=bpm, ri=ri, qtab=qtab, dht=dht, sel=sel, seg_first=seg_first,
                seg_end=seg_end, scan=scan, n_mcu=n_mcu)


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


def _read(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    with open(src, 'rb') as fh:
        return fh.read()


def _host_decode(src):
    from .data.im_worker import load_bgr
    return load_bgr(io.BytesIO(src) if isinstance(src, (bytes, bytearray, memoryview)) else src)


def _status_reason(word):
    for bit, name in STATUS_BITS:
        if word & bit:
            return 'damaged_' + name
    return 'damaged'


def decode_jpeg(sources, timing=None, sub=None, split_passes=False):
    """sources: paths or bytes -> a list of (H, W, 3) uint8 BGR device tensors, in order; every tensor owns its storage.  What the device
    does not decode (parse_jpeg's fallbacks, streams the kernels flag) comes through load_bgr, which may raise as it does today.
    timing: a dict that collects the stages in seconds, each closed by a synchronise; 'rounds' gets the rounds of every segment.
    sub: the subsequence size in bytes (default: sn_jpeg_limits); split_passes: the rounds and the write pass as two launches (timing)."""
    import torch
    from . import hip
    dev = hip.require_gpu()
    sources = list(sources)
    out = [None] * len(sources)
    t0 = time.perf_counter()
    blobs = [_read(s) for s in sources]
    t0 = _lap(timing, 'read_s', t0, sync=False)
    heads = [parse_jpeg(b) for b in blobs]
    t0 = _lap(timing, 'parse_s', t0, sync=False)
    lim = jpeg_limits()
    sub = int(sub or lim['sub'])
    for i, h in enumerate(heads):
        # a segment is decoded by one workgroup, at the worst in one round per subsequence: the longest scans stay on the host
        if 'fallback' not in h and int((h['seg_end'] - h['seg_first']).max()) > MAX_SEGMENT_SUBS * sub:
            heads[i] = _fallback('long_scan')
    todo = [i for i, h in enumerate(heads) if 'fallback' not in h]
    # batches whose pooled sizes stay below 2^30 (the kernels index with 32 bits); one batch for any ordinary call
    start = 0
    while start < len(todo):
        stop, nbytes, npix = start, 0, 0
        while stop < len(todo) and stop - start < lim['max_images']:
            h = heads[todo[stop]]
            b, p = len(blobs[todo[stop]]), h['mcux'] * h['mcuy'] * h['bpm'] * 64
            if stop > start and (nbytes + b > (1 << 30) or npix + p > (1 << 29)):
                break
            nbytes, npix, stop = nbytes + b, npix + p, stop + 1
        _decode_batch([todo[i] for i in range(start, stop)], blobs, heads, out, timing, sub, split_passes, dev)
        start = stop
    t0 = time.perf_counter()
    for i, h in enumerate(heads):
        if out[i] is None:
            _count(h.get('fallback') or h['flagged'])
            out[i] = hip.dev(_host_decode(sources[i]))
    _lap(timing, 'fallback_s', t0)
    return out


def _decode_batch(idx, blobs, heads, out, timing, sub, split_passes, dev):
    import torch
    from . import hip
    t0 = time.perf_counter()
    I = len(idx)
    img = np.zeros((I, IMG_FIELDS), np.int32)
    segs, qtab, dht = [], np.zeros((I, 3, 64), np.uint16), np.zeros((I, 4, DHT_BYTES), np.uint8)
    stream0 = blk0 = plane0 = sub0 = seg0 = 0
    for j, i in enumerate(idx):
        h = heads[i]
        nseg = len(h['seg_first'])
        nblk = h['n_mcu'] * h['bpm']
        img[j] = (h['W'], h['H'], h['ncomp'], h['hs'], h['vs'], h['mcux'], h['mcuy'], h['bpm'], seg0, nseg, blk0, plane0, stream0, len(blobs[i]),
                  h['sel'], h['ri'])
        s = np.zeros((nseg, SEG_FIELDS), np.int32)
        nsub = np.maximum(1, -(-(h['seg_end'] - h['seg_first']) // sub))
        s[:, 0], s[:, 1], s[:, 2] = j, h['seg_first'], h['seg_end']
        s[:, 3] = sub0 + np.concatenate([[0], np.cumsum(nsub)[:-1]])
        s[:, 4] = nsub
        segs.append(s)
        qtab[j, :h['ncomp']] = h['qtab']
        dht[j] = h['dht']
        seg0 += nseg
        sub0 += int(nsub.sum())
        blk0 += nblk
        plane0 += _align(nblk * 64)
        stream0 += _align(len(blobs[i]))
    seg = np.concatenate(segs)
    S, n_sub, n_blocks, plane_bytes, total = seg0, sub0, blk0, plane0, stream0
    # one upload: the tables, then the streams
    parts = [img.view(np.uint8).reshape(-1), seg.view(np.uint8).reshape(-1), qtab.view(np.uint8).reshape(-1), dht.reshape(-1)]
    offs, at = [], 0
    for p in parts:
        offs.append(at)
        at += _align(p.size)
    ptr_off = at
    at += _align(8 * I)
    data_off = at
    host = np.zeros(at + total, np.uint8)
    for p, o in zip(parts, offs):
        host[o:o + p.size] = p
    for j, i in enumerate(idx):
        o = data_off + int(img[j, 12])
        host[o:o + len(blobs[i])] = np.frombuffer(blobs[i], np.uint8)
    tensors = [torch.empty((int(img[j, 1]), int(img[j, 0]), 3), dtype=torch.uint8, device=dev) for j in range(I)]
    host[ptr_off:ptr_off + 8 * I] = np.array([t.data_ptr() for t in tensors], np.uint64).view(np.uint8)
    t0 = _lap(timing, 'tables_s', t0, sync=False)
    blob = torch.from_numpy(host).to(dev)
    d_img, d_seg, d_qtab, d_dht = (blob[o:] for o in offs)
    d_ptr, d_data = blob[ptr_off:], blob[data_off:]
    state = torch.empty((3, n_sub, 2), dtype=torch.int32, device=dev)
    counts = torch.empty((2, n_sub), dtype=torch.int32, device=dev)
    rounds = torch.empty((S,), dtype=torch.int32, device=dev)
    status = torch.zeros((I,), dtype=torch.int32, device=dev)
    coef = torch.zeros((n_blocks, 64), dtype=torch.int16, device=dev)
    planes = torch.empty((plane_bytes,), dtype=torch.uint8, device=dev)
    t0 = _lap(timing, 'upload_s', t0)
    st = hip.stream()
    ent = lambda phases: hip.call('sn_jpeg_entropy', d_data, total, d_img, img, I, d_seg, seg, S, d_dht, sub, n_sub, n_blocks, state, counts,
                                  coef, rounds, status, phases, st)
    if split_passes or timing is not None:
        ent(1)
        t0 = _lap(timing, 'rounds_s', t0)
        ent(2)
        t0 = _lap(timing, 'write_s', t0)
    else:
        ent(3)
    hip.call('sn_jpeg_dc', d_img, img, I, d_seg, seg, S, n_blocks, coef, status, st)
    t0 = _lap(timing, 'dc_s', t0)
    hip.call('sn_jpeg_pixels', d_img, img, I, d_qtab, coef, n_blocks, planes, plane_bytes, d_ptr, status, st)
    t0 = _lap(timing, 'pixels_s', t0)
    h_status = status.cpu().numpy()          # the one read-back (the sizes are the host's already: the frame headers)
    if timing is not None:
        timing.setdefault('rounds', []).extend(int(v) for v in rounds.cpu().numpy())
    _lap(timing, 'status_s', t0)
    good = 0
    for j, i in enumerate(idx):
        if h_status[j] == 0:
            out[i] = tensors[j]
            good += 1
        else:
            heads[i]['flagged'] = _status_reason(int(h_status[j]))
    _count('device', good)
