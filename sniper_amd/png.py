"""PNG files from pictures on the device (csrc/png_encode.hip): the row filters, a deflate coder with run
matches and per-block Huffman codes, and the container.  A rendered batch (visualization.render_lists of device tensors) is encoded
without its raw bytes leaving HBM: what comes to the host is one read-back of the stream lengths and the compressed bytes.

    deflate_streams(buffers)          zlib streams (RFC 1950) of byte buffers: any decoder's zlib.decompress gives the buffers back
    png_filter(pictures)              the filtered streams of (h, w, 3) uint8 pictures, on the device
    encode_png(pictures)              the files' bytes
    write_png(paths, pictures)        the files

The host's share: the chunk framing and its CRC-32 (zlib.crc32), the file writes."""
import ctypes
import struct
import time
import zlib

import numpy as np

__all__ = ['deflate_streams', 'png_filter', 'encode_png', 'write_png', 'png_container', 'deflate_bound', 'deflate_limits']

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'
_LIMITS = []


def deflate_limits():
    """sn_deflate_limits -> dict: block (the bytes B of a deflate block), threads, max_streams, code_words, code_lds, write_lds"""
    if not _LIMITS:
        from ._lib import lib
        out = (ctypes.c_int32 * 6)()
        lib().call('sn_deflate_limits', out)
        _LIMITS.append(dict(zip(('block', 'threads', 'max_streams', 'code_words', 'code_lds', 'write_lds'), (int(v) for v in out))))
    return _LIMITS[0]


def deflate_bound(n, block=None):
    """the most bytes of the zlib stream of n input bytes: n + 5 * (nb + 1) + 6 with nb = ceil(n / B)"""
    B = int(block) if block else deflate_limits()['block']
    nb = -(-int(n) // B)
    return int(n) + 5 * (nb + 1) + 6


def _chunk(kind, body):
    """the pieces of one chunk: length, type, data, CRC-32 of type and data (the data is not copied: any buffer)"""
    return (struct.pack('>I', len(body)), kind, body, struct.pack('>I', zlib.crc32(body, zlib.crc32(kind)) & 0xffffffff))


def png_container(h, w, zstream):
    """signature, IHDR (8 bits, colour type 2 = RGB, no interlace), ONE IDAT holding the zlib stream of the filtered rows, IEND;
    zstream: bytes or any contiguous buffer (copied once, into the file's bytes)"""
    body = memoryview(zstream).cast('B')
    return b''.join((PNG_SIGNATURE,) + _chunk(b'IHDR', struct.pack('>IIBBBBB', int(w), int(h), 8, 2, 0, 0, 0)) + _chunk(b'IDAT', body) +
                    _chunk(b'IEND', b''))


def _lap(timing, key, t0):
    if timing is None:
        return t0
    import torch
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    timing[key] = timing.get(key, 0.0) + t1 - t0
    return t1


def _deflate_device(data, offsets, timing=None):
    """data: uint8 device tensor; offsets: HOST int64 (S+1) -> (host uint8 array of the compact streams, out_off (S+1) int64)"""
    import torch
    from . import hip
    dev = hip.require_gpu()
    lim = deflate_limits()
    h_off = np.ascontiguousarray(offsets, np.int64)
    S = len(h_off) - 1
    if S < 1 or S > lim['max_streams']:
        raise ValueError('deflate_streams: %d streams, 1 .. %d per call' % (S, lim['max_streams']))
    total = int(h_off[-1])
    sizes = np.diff(h_off)
    B = lim['block']
    n_blocks = int(np.where(sizes > 0, -(-sizes // B), 1).sum())
    capacity = int(sum(deflate_bound(int(n), B) for n in sizes))
    t0 = time.perf_counter()
    d_off = hip.dev(h_off)
    blk_first = torch.empty((S + 1,), dtype=torch.int32, device=dev)
    blk_code = torch.empty((n_blocks, lim['code_words']), dtype=torch.int32, device=dev)
    blk_size = torch.empty((n_blocks,), dtype=torch.int64, device=dev)
    out = torch.empty((capacity,), dtype=torch.uint8, device=dev)
    st = hip.stream()
    hip.call('sn_deflate_plan', d_off, h_off, S, total, blk_first, st)
    hip.call('sn_deflate_code', data if total else None, d_off, h_off, S, total, blk_first, n_blocks, blk_code, blk_size, st)
    t0 = _lap(timing, 'code_s', t0)
    ends = torch.cumsum(blk_size, 0)
    blk_pos = ends - blk_size
    # stream s starts at blk_pos[blk_first[s]]; the last entry is the total
    out_off = torch.cat([blk_pos, ends[-1:]])[blk_first.long()]
    t0 = _lap(timing, 'scan_s', t0)
    hip.call('sn_deflate_write', data if total else None, d_off, h_off, S, total, blk_first, n_blocks, blk_code, blk_pos, out, capacity, st)
    t0 = _lap(timing, 'write_s', t0)
    h_out_off = out_off.cpu().numpy()          # the one read-back before the download: S + 1 offsets
    t0 = _lap(timing, 'lengths_s', t0)
    n_out = int(h_out_off[-1])
    if n_out > capacity or (np.diff(h_out_off) > np.array([deflate_bound(int(n), B) for n in sizes])).any():
        raise RuntimeError('deflate_streams: a stream is longer than its bound (%d bytes for a capacity of %d)' % (n_out, capacity))
    host = out[:n_out].cpu().numpy()
    _lap(timing, 'download_s', t0)
    return host, h_out_off


def deflate_streams(buffers, offsets=None, timing=None):
    """buffers: a list of bytes-likes / uint8 arrays, or (with `offsets`, (S+1) int64 on the host) one uint8 device tensor or array
    holding S streams back to back -> one zlib stream (bytes) per input stream."""
    import torch
    from . import hip
    if offsets is None:
        arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8).reshape(-1) for b in buffers]
        offsets = np.concatenate([[0], np.cumsum([a.size for a in arrs])]).astype(np.int64)
        flat = np.concatenate(arrs) if len(arrs) and offsets[-1] else np.zeros(0, np.uint8)
        data = hip.dev(flat) if flat.size else torch.empty((0,), dtype=torch.uint8, device=hip.require_gpu())
    else:
        data = hip.dev(buffers).reshape(-1)
        if data.dtype != torch.uint8:
            raise ValueError('deflate_streams: uint8 data required, got %s' % data.dtype)
        offsets = np.ascontiguousarray(offsets, np.int64)
        if offsets[-1] != data.numel():
            raise ValueError('deflate_streams: the offsets end at %d, the data has %d bytes' % (offsets[-1], data.numel()))
    host, off = _deflate_device(data, offsets, timing)
    return [host[off[s]:off[s + 1]].tobytes() for s in range(len(off) - 1)]


def _pack_pictures(pictures):
    """-> (flat uint8 device tensor, hw (I, 2) int64, pix_off (I+1) int64)"""
    import torch
    from . import hip
    I = len(pictures)
    if I < 1:
        raise ValueError('png: no pictures')
    for p in pictures:
        if len(p.shape) != 3 or int(p.shape[2]) != 3 or not str(p.dtype).endswith('uint8') or min(int(p.shape[0]), int(p.shape[1])) < 1:
            raise ValueError('png: (h, w, 3) uint8 pictures required, got %s %s' % (tuple(p.shape), p.dtype))
    hw = np.array([[int(p.shape[0]), int(p.shape[1])] for p in pictures], np.int64).reshape(-1, 2)
    pix_off = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])]).astype(np.int64)
    if all(isinstance(p, torch.Tensor) and p.is_cuda for p in pictures):
        flat = [p.contiguous().reshape(-1) for p in pictures]
        src = flat[0] if I == 1 else torch.cat(flat)          # (a device-to-device copy: the pictures stay in HBM)
    else:
        host = [p.cpu().numpy() if isinstance(p, torch.Tensor) else np.ascontiguousarray(p, np.uint8) for p in pictures]
        src = hip.dev(np.concatenate([h.reshape(-1) for h in host]))
    return src, hw, pix_off


def png_filter(pictures, timing=None):
    """pictures: (h, w, 3) uint8 RGB, numpy arrays or device tensors, sizes may differ -> (streams, offsets): one uint8 device tensor
    holding picture i's filtered rows (a filter-type byte and 3 * w bytes per row) at offsets[i] .. offsets[i+1], offsets on the host."""
    import torch
    from . import hip
    dev = hip.require_gpu()
    t0 = time.perf_counter()
    src, hw, pix_off = _pack_pictures(pictures)
    I = len(hw)
    stream_off = np.concatenate([[0], np.cumsum(hw[:, 0] * (3 * hw[:, 1] + 1))]).astype(np.int64)
    hw32 = np.ascontiguousarray(hw, np.int32)
    t0 = _lap(timing, 'upload_s', t0)
    out = torch.empty((int(stream_off[-1]),), dtype=torch.uint8, device=dev)
    hip.call('sn_png_filter', src, hip.dev(hw32), hw32, hip.dev(pix_off), hip.dev(stream_off), I, int(pix_off[-1]), int(stream_off[-1]), out,
             hip.stream())
    _lap(timing, 'filter_s', t0)
    return out, stream_off


def encode_png(pictures, timing=None):
    """-> the bytes of one PNG file per picture (8-bit RGB, adaptive row filters, one IDAT)"""
    streams, off = png_filter(pictures, timing)
    host, zoff = _deflate_device(streams, off, timing)
    t0 = time.perf_counter()
    files = [png_container(int(p.shape[0]), int(p.shape[1]), host[zoff[i]:zoff[i + 1]]) for i, p in enumerate(pictures)]
    if timing is not None:
        timing['container_s'] = timing.get('container_s', 0.0) + time.perf_counter() - t0
    return files


def write_png(paths, pictures, timing=None):
    """encode_png, then one file per picture"""
    paths = list(paths)
    if len(paths) != len(pictures):
        raise ValueError('write_png: %d paths for %d pictures' % (len(paths), len(pictures)))
    files = encode_png(pictures, timing)
    t0 = time.perf_counter()
    for path, data in zip(paths, files):
        with open(path, 'wb') as fh:
            fh.write(data)
    if timing is not None:
        timing['file_s'] = timing.get('file_s', 0.0) + time.perf_counter() - t0
    return paths
