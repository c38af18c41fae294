"""Fixtures of the JPEG tests, made at test time with PIL's encoder: pictures, files, PIL's own decode (the yardstick)."""
import io

import numpy as np

SAMPLINGS = (('444', 0), ('422', 1), ('420', 2), ('grey', None))
VARIANTS = (('plain', {}), ('optimize', {'optimize': True}), ('rst_mcu', {'restart_marker_blocks': 1}), ('rst_row', {'restart_marker_rows': 1}))


def picture(kind, h, w, seed=0):
    """(h, w, 3) uint8 RGB: 'smooth' (ramps), 'noise' (uniform), 'harsh' (black and white) or 'lowpass' (noise blurred: photograph-like
    statistics)"""
    rng = np.random.default_rng(seed + 1000 * h + w)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == 'harsh':          # black and white 8 x 8 blocks in turn, a quarter of the pixels flipped: the largest DC differences there are
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.where(((yy // 8 + xx // 8) % 2 == 0) ^ (rng.random((h, w)) < 0.25), 255, 0).astype(np.uint8)
        return np.stack([a, a, np.where(rng.random((h, w)) < 0.5, a, 255 - a).astype(np.uint8)], 2)
    if kind == 'lowpass':
        a = rng.integers(0, 256, (h + 8, w + 8, 3)).astype(np.float64)
        for ax in (0, 1):
            c = np.cumsum(a, axis=ax)
            a = (np.take(c, range(8, a.shape[ax]), axis=ax) - np.take(c, range(0, a.shape[ax] - 8), axis=ax)) / 8.0
        a = (a - a.min()) / max(a.max() - a.min(), 1e-9) * 255.0
        return a[:h, :w].astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(yy * 7 + xx * 3) % 256, (xx * 5 + 40) % 256, (yy * 2 + xx * 2 + 90) % 256], 2).astype(np.uint8)


def encode(arr, sampling=0, quality=75, **kw):
    """the bytes of a JPEG file of an RGB picture; sampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0, None = grey (the first channel)"""
    from PIL import Image
    buf = io.BytesIO()
    if sampling is None:
        Image.fromarray(arr[:, :, 0]).save(buf, 'JPEG', quality=quality, **kw)
    else:
        Image.fromarray(arr).save(buf, 'JPEG', quality=quality, subsampling=sampling, **kw)
    return buf.getvalue()


def pil_bgr(data):
    """what data.im_worker.load_bgr gives for these bytes"""
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[:, :, ::-1])


def scan_range(data):
    """(first byte of the entropy-coded data, the index of the EOI marker)"""
    from sniper_amd.jpeg import parse_jpeg
    head = parse_jpeg(data)
    return int(head['scan']), int(head['seg_end'][-1])


def small_damaged_streams():
    """(name, bytes) of the damaged files the CPU program and the GPU tests share: one truncated inside the scan, one with a byte
    overwritten inside the scan, one whose frame header claims more rows than the scan holds"""
    import jpeg_ref
    data = encode(picture('noise', 24, 40, seed=5), 2, 90)
    first, end = scan_range(data)
    cut = data[:first + (end - first) // 2]
    # (a prefix code finds its way back after most single errors, and the stream stays a sound one with other coefficients: the byte
    # taken is the first from a third of the scan on whose change the restatement cannot decode)
    from sniper_amd.jpeg import parse_jpeg
    for at in range(first + (end - first) // 3, end):
        over = bytearray(data)
        over[at] ^= 0x5a
        head = parse_jpeg(bytes(over))
        if 'fallback' in head:
            continue
        try:
            jpeg_ref.coefficients(head, bytes(over))
        except (ValueError, IndexError):
            break
    else:
        raise AssertionError('no byte of the scan damages the stream')
    tall = bytearray(data)
    at = data.index(b'\xff\xc0')
    assert tall[at + 5:at + 7] == bytes([0, 24])
    tall[at + 5:at + 7] = bytes([0, 72])          # SOF: 72 rows instead of 24
    return [('truncated', bytes(cut)), ('overwritten', bytes(over)), ('more_blocks', bytes(tall))]
