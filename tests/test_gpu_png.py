"""GPU: the deflate coder, the PNG row filters and the encoder (sniper_amd/png.py, csrc/png_encode.hip).  Every coded stream is
decoded by an independent decoder -- zlib.decompress or PIL -- and compared with == / np.array_equal against the input; the filtered
streams are compared byte for byte with the numpy restatement tests/png_ref.py."""
import io
import os
import zlib

import numpy as np
import pytest

import png_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def png():
    from sniper_amd import png as mod
    return mod


@pytest.fixture(scope='module')
def B(png):
    return png.deflate_limits()['block']


def _roundtrip(png, B, buffers):
    outs = png.deflate_streams(buffers)
    assert len(outs) == len(buffers)
    for src, z in zip(buffers, outs):
        src = bytes(src)
        assert z[:2] == b'\x78\x01'
        assert zlib.decompress(z) == src
        assert len(z) <= png_ref.deflate_bound(len(src), B), (len(z), len(src))
    return outs


def _distinct(n, seed):
    """n bytes, no two neighbours equal"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 255, n).astype(np.int64)
    for i in range(1, n):
        if a[i] == a[i - 1]:
            a[i] = (a[i] + 1) % 255
    return a.astype(np.uint8)


# ---- deflate on arbitrary bytes ----------------------------------------------------------------------------------------------------
def test_lengths_around_the_block_size(png, B):
    rng = np.random.default_rng(0)
    text = (rng.integers(0, 8, 2 * B + 1) * 31).astype(np.uint8)          # compressible: the dynamic path
    bufs = [text[:n].tobytes() for n in (0, 1, 2, 3, B - 1, B, B + 1, 2 * B, 2 * B + 1)]
    outs = _roundtrip(png, B, bufs)
    assert len(outs[0]) == 11 and outs[0] == zlib.compress(b'', 0)          # one final empty stored block
    assert len(outs[-1]) < len(bufs[-1]) // 2


def test_ragged_batch_with_empty_streams(png, B):
    rng = np.random.default_rng(1)
    bufs = [b'', bytes(rng.integers(0, 3, 700).astype(np.uint8)), b'', b'\x00', bytes(rng.integers(0, 256, B + 17).astype(np.uint8)), b'',
            bytes(1000), b'']
    _roundtrip(png, B, bufs)


def test_device_bytes_and_offsets_form(png, B):
    import torch
    rng = np.random.default_rng(2)
    flat = rng.integers(0, 5, 3 * B + 100).astype(np.uint8)
    off = np.array([0, 5, 5, B + 5, 3 * B + 100], np.int64)
    outs = png.deflate_streams(torch.as_tensor(flat).cuda(), off)
    for s in range(4):
        assert zlib.decompress(outs[s]) == flat[off[s]:off[s + 1]].tobytes()


def test_all_byte_values(png, B):
    a = np.tile(np.arange(256, dtype=np.uint8), 40)                         # both halves of the literal alphabet, equal counts
    b = np.repeat(np.arange(256, dtype=np.uint8), 3)                        # runs of exactly 3 of every value
    _roundtrip(png, B, [a.tobytes(), b.tobytes(), a[::-1].tobytes()])


@pytest.mark.parametrize('run', [2, 3, 4, 257, 258, 259, 260, 261, 517])
def test_run_lengths_between_distinct_neighbours(png, B, run):
    body = b'\x05' + b'\x09' * run + b'\x05' + _distinct(300, run).tobytes() + b'\xfe' * run + b'\x01'
    # between distinct neighbours, and as a whole stream (the run then starts on the block's first byte and ends on its last)
    _roundtrip(png, B, [body, b'\x09' * run])
    # what the restatement makes of the first run: a literal, then pieces of 258; a piece of 1 or 2 bytes is literals
    toks = png_ref.tokens(b'\x05' + b'\x09' * run + b'\x05')
    want = {2: 0, 3: 0, 4: 1, 257: 1, 258: 1, 259: 1, 260: 1, 261: 1, 517: 2}[run]
    assert sum(1 for k, _ in toks if k == 'm') == want


def test_run_placement(png, B):
    base = _distinct(2 * B + 500, 5)
    first = base.copy()
    first[B:B + 40] = 7                     # a run that starts on the first byte of the second block
    first[B - 1] = 8
    straddle = base.copy()
    straddle[B - 300:B + 300] = 9           # a run across the block boundary: no match reaches back over it
    tail = base.copy()
    tail[-77:] = 3                          # a run that ends on the last byte of the stream
    head = base.copy()
    head[:600] = 4                          # a run from the first byte of the stream
    outs = _roundtrip(png, B, [first.tobytes(), straddle.tobytes(), tail.tobytes(), head.tobytes()])
    assert all(len(z) > 0 for z in outs)


def test_one_value_block_and_block_without_runs(png, B):
    one = b'\x2a' * B                       # the code: that literal, length symbols, 256
    none = _distinct(B, 11) % 16            # no run at all: no distance code
    none = none.astype(np.uint8)
    for i in range(1, len(none)):
        if none[i] == none[i - 1]:
            none[i] = (none[i] + 1) % 16
    assert all(k == 'l' for k, _ in png_ref.tokens(none.tobytes()))
    outs = _roundtrip(png, B, [one, none.tobytes(), one + none.tobytes()])
    assert len(outs[0]) < 120 and len(outs[1]) < 0.6 * B


def test_length_limit_fibonacci_counts(png, B):
    counts = [1, 3]
    while len(counts) < 16:
        counts.append(counts[-1] + counts[-2])
    data = png_ref.spread(counts)
    assert len(data) == 5775 and len(data) < B and np.bincount(data).tolist() == counts
    assert all(k == 'l' for k, _ in png_ref.tokens(data.tobytes()))                      # no runs
    assert png_ref.huffman_depth(counts + [1]) == 16                                    # the unlimited code is deeper than 15
    z = _roundtrip(png, B, [data.tobytes()])[0]
    assert len(z) < len(data) // 2                                                      # the dynamic path, not the stored one


def test_random_bytes_take_the_stored_path(png, B):
    rng = np.random.default_rng(4)
    n = 3 * B
    data = rng.integers(0, 256, n).astype(np.uint8).tobytes()
    z = _roundtrip(png, B, [data])[0]
    nb = 3
    assert n <= len(z) <= n + 5 * (nb + 1) + 6
    assert len(z) == 2 + 3 * (B + 5) + 4


def test_two_runs_give_identical_bytes(png, B):
    rng = np.random.default_rng(6)
    bufs = [bytes(rng.integers(0, 6, 2 * B + 9).astype(np.uint8)), b'', bytes(5000), bytes(rng.integers(0, 256, 4000).astype(np.uint8))]
    assert png.deflate_streams(bufs) == png.deflate_streams(bufs)


# ---- derived size caps ---------------------------------------------------------------------------------------------------------------
def test_size_cap_zero_bytes(png, B):
    n = 1 << 20
    z = _roundtrip(png, B, [bytes(n)])[0]
    print('2^20 zero bytes -> %d bytes (%.5f)' % (len(z), len(z) / n))
    assert len(z) <= 0.01 * n


def test_size_cap_four_values(png, B):
    n = 1 << 20
    data = np.random.default_rng(7).integers(0, 4, n).astype(np.uint8).tobytes()
    z = _roundtrip(png, B, [data])[0]
    print('2^20 bytes of four values -> %d bytes (%.5f)' % (len(z), len(z) / n))
    assert len(z) <= 0.30 * n


# ---- the filter ----------------------------------------------------------------------------------------------------------------------
def _filter_equal(png, pics):
    streams, off = png.png_filter(pics)
    host = streams.cpu().numpy()
    assert off[-1] == host.size
    for i, p in enumerate(pics):
        p = p.cpu().numpy() if hasattr(p, 'cpu') else p
        assert np.array_equal(host[off[i]:off[i + 1]], png_ref.filter_picture(p)), 'picture %d %s' % (i, p.shape)


def test_filter_tiny_and_narrow_pictures(png):
    rng = np.random.default_rng(8)
    shapes = [(1, 1), (1, 5), (5, 1), (4, 2), (4, 3), (3, 4), (7, 21), (6, 22), (3, 100)]          # 3w = 63, 66, 300: around 64 lanes
    _filter_equal(png, [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes])


def test_filter_small_amplitude_noise_and_values_near_255(png):
    rng = np.random.default_rng(9)
    smooth = (120 + rng.integers(-3, 4, (40, 70, 3))).astype(np.uint8)          # neighbours within a few levels: all Paeth branches
    high = (250 + rng.integers(0, 6, (33, 45, 3))).astype(np.uint8)             # the 9-bit Average sum, wrap-around
    mixed = np.where(rng.random((20, 50, 3)) < 0.5, 255, 0).astype(np.uint8)
    _filter_equal(png, [smooth, high, mixed])


def _five_winners():
    """a picture in which each of the five filters wins at least one row"""
    rng = np.random.default_rng(10)
    w = 48
    rows = []
    rows.append(np.where(rng.random((w, 3)) < 0.5, 0, 1).astype(np.int64) * np.array([1, 255, 1]))          # None: bytes already near 0 / 256
    rows.append((np.arange(w)[:, None] * 5 + np.array([0, 60, 120])) % 256)                                # Sub: a horizontal ramp
    rows.append(rows[-1].copy())                                                                          # Up: the row above again
    noise = rng.integers(0, 256, (w, 3))
    rows.append(noise)
    avg = np.zeros((w, 3), np.int64)                                                                      # Average: exactly (left + up) >> 1
    for x in range(w):
        left = avg[x - 1] if x else np.zeros(3, np.int64)
        avg[x] = (left + noise[x]) >> 1
    rows.append(avg)
    up = rng.integers(0, 256, (w, 3))
    rows.append(up)
    pa = np.zeros((w, 3), np.int64)               # Paeth: the predictor, and a step of 40 at every fifth pixel (without the steps the
    for x in range(w):                            # row would repeat the one above, and Up would tie)
        a = pa[x - 1] if x else np.zeros(3, np.int64)
        c = up[x - 1] if x else np.zeros(3, np.int64)
        pa[x] = (png_ref.paeth_predictor(a, up[x], c) + (40 if x % 5 == 2 else 0)) % 256
    rows.append(pa)
    return np.stack(rows).astype(np.uint8)


def test_filter_every_type_wins_a_row(png):
    pic = _five_winners()
    _, types = png_ref.filter_picture(pic, want_types=True)
    assert set(types) == {0, 1, 2, 3, 4}, types
    _filter_equal(png, [pic])


def test_filter_ragged_batch_of_device_tensors(png):
    import torch
    rng = np.random.default_rng(12)
    pics = [torch.as_tensor(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).cuda() for h, w in ((9, 130), (2, 3), (31, 64), (1, 200))]
    _filter_equal(png, pics)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _decode(data):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.mode == 'RGB'
    return np.asarray(im)


def test_encode_one_pixel(png):
    pic = np.array([[[7, 200, 31]]], np.uint8)
    data = png.encode_png([pic])[0]
    assert data[:8] == b'\x89PNG\r\n\x1a\n' and data.count(b'IDAT') == 1
    assert np.array_equal(_decode(data), pic)


def test_encode_streams_of_exactly_a_block(png, B):
    # a filtered stream is h * (3w + 1) bytes: the narrowest picture whose stream has exactly the length wanted
    rng = np.random.default_rng(13)
    shapes = []
    for target in (B, B - 1, B + 1):
        found = None
        for w in range(1, 2000):
            if target % (3 * w + 1) == 0:
                found = (target // (3 * w + 1), w)
                break
        assert found is not None, target
        shapes.append(found)
    pics = [(rng.integers(0, 4, (h, w, 3)) * 60).astype(np.uint8) for h, w in shapes]
    streams, off = png.png_filter(pics)
    assert np.diff(off).tolist() == [B, B - 1, B + 1]
    for pic, data in zip(pics, png.encode_png(pics)):
        assert np.array_equal(_decode(data), pic)


def test_encode_ragged_batch_and_write(png, tmp_path):
    import torch
    from PIL import Image
    rng = np.random.default_rng(14)
    yy, xx = np.mgrid[0:120, 0:160]
    smooth = np.stack([(yy + xx) % 256, (2 * yy) % 256, (xx * xx // 97) % 256], -1).astype(np.uint8)
    pics = [smooth, rng.integers(0, 256, (37, 53, 3)).astype(np.uint8), np.full((64, 64, 3), 90, np.uint8), np.zeros((1, 7, 3), np.uint8)]
    for data, pic in zip(png.encode_png(pics), pics):
        assert np.array_equal(_decode(data), pic)
    paths = [str(tmp_path / ('p%d.png' % i)) for i in range(len(pics))]
    png.write_png(paths, [torch.as_tensor(p).cuda() for p in pics])
    for path, pic in zip(paths, pics):
        assert np.array_equal(np.asarray(Image.open(path)), pic)


def _roidb(tmp_path, n=3):
    from PIL import Image
    rng = np.random.default_rng(15)
    roidb = []
    for i in range(n):
        h, w = 60 + 11 * i, 90 + 7 * i
        path = str(tmp_path / ('src%d.png' % i))
        Image.fromarray(rng.integers(0, 256, (h, w, 3)).astype(np.uint8)).save(path)
        roidb.append({'image': path, 'flipped': i == 1, 'height': h, 'width': w})
    boxes = [[[] for _ in range(n)] for _ in range(3)]
    for j in (1, 2):
        for i in range(n):
            boxes[j][i] = np.array([[5 + 3 * j, 6, 50 + i, 40 + j, 0.9], [20, 22, 70, 55, 0.3]], np.float32)
    return roidb, boxes


def test_render_results_device_encoder_matches_pil(tmp_path):
    from PIL import Image
    from sniper_amd.visualization import render_results
    roidb, boxes = _roidb(tmp_path)
    names = ['__background__', 'cat', 'dog']
    a = render_results(roidb, boxes, names, str(tmp_path / 'pil'))
    b = render_results(roidb, boxes, names, str(tmp_path / 'dev'), encoder='device')
    assert len(a) == len(b) == 3
    for pa, pb in zip(a, b):
        assert os.path.basename(pa) == os.path.basename(pb)
        assert np.array_equal(np.asarray(Image.open(pa)), np.asarray(Image.open(pb)))
        with open(pb, 'rb') as fh:
            assert fh.read().count(b'IDAT') == 1          # this project's container, not PIL's
    # another extension still goes through PIL: the same bytes as the default encoder writes
    c = render_results(roidb, boxes, names, str(tmp_path / 'pil_bmp'), vis_ext='.bmp')
    d = render_results(roidb, boxes, names, str(tmp_path / 'dev_bmp'), vis_ext='.bmp', encoder='device')
    for pc, pd in zip(c, d):
        with open(pc, 'rb') as f1, open(pd, 'rb') as f2:
            assert f1.read() == f2.read()
    # '.PNG' is a PNG too
    e = render_results(roidb, boxes, names, str(tmp_path / 'dev_upper'), vis_ext='.PNG', encoder='device')
    assert np.array_equal(np.asarray(Image.open(e[0])), np.asarray(Image.open(a[0])))


def test_visualize_dets_device_encoder(tmp_path):
    from PIL import Image
    from sniper_amd.visualization import visualize_dets
    rng = np.random.default_rng(16)
    im = rng.integers(0, 256, (50, 80, 3)).astype(np.uint8)
    dets = [[], np.array([[4, 5, 60, 40, 0.8]], np.float32)]
    p1, p2 = str(tmp_path / 'a.png'), str(tmp_path / 'b.png')
    pic1 = visualize_dets(im, dets, 1.0, None, ['bg', 'thing'], save_path=p1, transform=False)
    pic2 = visualize_dets(im, dets, 1.0, None, ['bg', 'thing'], save_path=p2, transform=False, encoder='device')
    assert np.array_equal(pic1, pic2)
    assert np.array_equal(np.asarray(Image.open(p1)), np.asarray(Image.open(p2)))
    with pytest.raises(ValueError):
        visualize_dets(im, dets, 1.0, None, ['bg', 'thing'], save_path=p2, transform=False, encoder='jpeg')


def test_tester_aggregate_vis_encoder_from_config(tmp_path):
    """Tester.aggregate(vis=True) reads cfg.TEST.VIS_ENCODER: the files of a 'device' run decode to the pixels of the default run"""
    from PIL import Image
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    rs = np.random.RandomState(21)
    roidb, _ = _roidb(tmp_path, 2)
    NC = 3

    def scale_dets():
        d = inference._Detections([[[] for _ in roidb] for _ in range(NC)])
        for i, e in enumerate(roidb):
            for j in range(1, NC):
                xy = rs.uniform(0, [e['width'] - 30, e['height'] - 25], (3, 2))
                wh = rs.uniform(8, 30, (3, 2))
                sc = rs.uniform(0.3, 1.0, (3, 1))
                d[j][i] = [np.hstack((xy, xy + wh, sc)).astype(np.float64)]
        return [d]

    class Imdb(object):
        num_classes, classes, name, result_path = NC, ['__background__', 'cat', 'dog'], 'synthetic', None
    dets = scale_dets()
    dirs = {}
    for encoder in (None, 'pil', 'device'):
        cfg = cfgmod.res101_e2e_autofocus()
        cfg.TEST.VALID_RANGES = ((-1, -1),)
        cfg.TEST.MAX_PER_IMAGE = 100
        if encoder is not None:
            cfg.TEST.VIS_ENCODER = encoder
        tester = inference.Tester(None, Imdb(), roidb, None, cfg=cfg, batch_size=1)
        dirs[encoder] = os.path.join(str(tmp_path), 'vis_%s' % encoder)
        tester.aggregate(dets, vis=True, cache_name=None, vis_path=dirs[encoder], vis_ext='.png')
    for i in range(len(roidb)):
        files = {}
        for encoder, d in dirs.items():
            with open(os.path.join(d, '%d.png' % i), 'rb') as fh:
                files[encoder] = fh.read()
        assert files[None] == files['pil']                  # 'pil' is the default and is the file of before
        assert files['device'] != files['pil'] and files['device'].count(b'IDAT') == 1
        assert np.array_equal(_decode(files['device']), _decode(files['pil']))
