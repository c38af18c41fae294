"""-m gpu: JPEG files decoded on the device (sniper_amd/jpeg.py, csrc/jpeg_decode.hip) against PIL's own decode of the same bytes --
torch.equal, nothing else: the small shapes at which the kernels can go wrong, long and custom codes, stuffed bytes on subsequence
boundaries, restart markers, ragged batches with fallbacks in the middle, damaged streams, and the wiring through DeviceImageCache,
im_worker, decode_ahead, MNIteratorE2E and the test-time wrapper."""
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_ref  # noqa: E402
from gpu_util import dev  # noqa: E402
from jpeg_util import SAMPLINGS, encode, picture, pil_bgr, scan_range, small_damaged_streams  # noqa: E402


def _assert_exact(got, datas, what=''):
    assert len(got) == len(datas)
    for i, (g, data) in enumerate(zip(got, datas)):
        want = torch.from_numpy(pil_bgr(data))
        assert g.is_cuda and g.dtype == torch.uint8 and tuple(g.shape) == tuple(want.shape), (what, i, g.shape, want.shape)
        assert torch.equal(g.cpu(), want), (what, i, int((g.cpu() != want).sum()))


@pytest.mark.parametrize('h,w', ((1, 1), (8, 8), (16, 16), (9, 17), (17, 33), (31, 3), (3, 31)))
def test_small_shapes_equal_pil(h, w):
    from sniper_amd import jpeg
    datas = [encode(picture(kind, h, w), samp, q) for kind in ('smooth', 'noise') for _, samp in SAMPLINGS for q in (30, 100)]
    jpeg.reset_stats()
    _assert_exact(jpeg.decode_jpeg(datas), datas, (h, w))
    st = jpeg.stats()
    if w <= 2:          # 4:2:2 and 4:2:0 of a picture two pixels wide or less: a chroma plane one sample wide, the host's
        assert st == {'device': 8, 'fallback': {'narrow_chroma': 8}}, st
    else:
        assert st == {'device': 16, 'fallback': {}}, st


def test_long_and_custom_codes_and_stuffed_bytes_on_boundaries():
    from sniper_amd import jpeg
    sub = jpeg.jpeg_limits()['sub']
    datas, on_zero, straddles, big = [], 0, 0, 0
    for seed in range(4):
        # optimize=True on noise: long codes of the file's own; quality 100 on black and white: magnitude categories of 10 and 11
        arr = picture('noise' if seed % 2 else 'harsh', 64, 96, seed=seed)
        for samp, kw in ((0, {'optimize': True}), (0, {}), (2, {'optimize': True})):
            data = encode(arr, samp, 100, **kw)
            datas.append(data)
            first, end = scan_range(data)
            assert b'\xff\x00' in data[first:end]
            head = jpeg.parse_jpeg(data)
            starts = []
            coef = jpeg_ref.coefficients(head, data, starts)
            big += int(np.abs(coef).max() >= 512)          # a category of 10 and more
            starts = set(starts)
            for at in range(first + sub, end, sub):
                on_zero += data[at] == 0 and data[at - 1] == 0xff
                straddles += (at * 8) not in starts
            if kw:
                assert max(int(np.flatnonzero(t[:16]).max()) + 1 for t in head['dht']) >= 12          # a code of 12 bits and more
    assert on_zero >= 1 and straddles >= 1 and big >= 3, (on_zero, straddles, big)
    jpeg.reset_stats()
    _assert_exact(jpeg.decode_jpeg(datas), datas)
    assert jpeg.stats() == {'device': len(datas), 'fallback': {}}


def test_restart_markers_short_streams_and_a_long_scan(capsys):
    from sniper_amd import jpeg
    sub = jpeg.jpeg_limits()['sub']
    datas = []
    for samp in (0, 1, 2, None):
        datas.append(encode(picture('noise', 40, 56), samp, 85, restart_marker_blocks=1))          # 12 - 35 intervals of one MCU
        datas.append(encode(picture('smooth', 160, 24), samp, 85, restart_marker_rows=1))          # 10 - 20 intervals of one MCU row
    for d in datas:
        assert len(jpeg.parse_jpeg(d)['seg_first']) > 8          # the marker numbers wrap
    tiny = encode(picture('smooth', 8, 8), None, 30)
    first, end = scan_range(tiny)
    assert end - first < sub                                    # a stream shorter than one subsequence
    datas.append(tiny)
    big = encode(picture('lowpass', 480, 640), 2, 75)
    first, end = scan_range(big)
    assert (end - first) // sub > 100                           # one scan of many subsequences
    datas.append(big)
    jpeg.reset_stats()
    timing = {}
    _assert_exact(jpeg.decode_jpeg(datas, timing=timing), datas)
    assert jpeg.stats() == {'device': len(datas), 'fallback': {}}
    rounds = timing['rounds']
    assert len(rounds) == sum(len(jpeg.parse_jpeg(d)['seg_first']) for d in datas)
    with capsys.disabled():
        print('\n480 x 640, 4:2:0, quality 75: %d subsequences of %d bytes, %d rounds' % (-(-(end - first) // sub), sub, rounds[-1]))
    assert 1 <= rounds[-1] <= -(-(end - first) // sub) and rounds[-2] == 1
    # other subsequence sizes decode alike, the smallest included
    for s in (16, 48, 1024):
        _assert_exact(jpeg.decode_jpeg(datas[-3:], sub=s), datas[-3:], s)


def test_ragged_batch_keeps_order_and_counts_fallbacks(tmp_path):
    from PIL import Image
    from sniper_amd import jpeg
    buf = io.BytesIO()
    Image.fromarray(picture('smooth', 30, 44)).save(buf, 'JPEG', progressive=True)
    progressive = buf.getvalue()
    buf = io.BytesIO()
    Image.fromarray(picture('noise', 21, 13)).save(buf, 'PNG')
    png = buf.getvalue()
    datas = [encode(picture('lowpass', 67, 101), 2, 75),
             encode(picture('noise', 9, 17), 0, 95, optimize=True),
             progressive,
             encode(picture('smooth', 48, 64), 1, 60, restart_marker_rows=1),
             png,
             encode(picture('noise', 33, 20), None, 50),
             encode(picture('lowpass', 120, 50), 2, 90, restart_marker_blocks=3, optimize=True),
             encode(picture('smooth', 2, 2), 2, 75)]
    sources = []
    for i, d in enumerate(datas):          # paths and bytes, mixed
        if i % 2:
            sources.append(d)
        else:
            path = str(tmp_path / ('f%d%s' % (i, '.png' if d is png else '.jpg')))
            with open(path, 'wb') as fh:
                fh.write(d)
            sources.append(path)
    jpeg.reset_stats()
    a = jpeg.decode_jpeg(sources)
    _assert_exact(a, datas)
    assert jpeg.stats() == {'device': 5, 'fallback': {'progressive': 1, 'not_jpeg': 1, 'narrow_chroma': 1}}
    b = jpeg.decode_jpeg(sources)
    assert all(torch.equal(x, y) and x.data_ptr() != y.data_ptr() for x, y in zip(a, b))
    assert jpeg.stats()['device'] == 10
    # every tensor owns its storage
    assert all(t.untyped_storage().nbytes() == t.numel() for t in a)


def test_damaged_streams_come_back_through_the_fallback():
    from sniper_amd import jpeg
    good = [encode(picture('lowpass', 40, 72), 2, 80), encode(picture('noise', 17, 33), 0, 90), encode(picture('smooth', 64, 64), 1, 70)]
    loads, raises = [], []
    for name, bad in small_damaged_streams():          # the bytes the sanitizer program has decoded on the CPU
        assert 'fallback' not in jpeg.parse_jpeg(bad), name
        try:
            pil_bgr(bad)
            loads.append((name, bad))
        except OSError:
            raises.append((name, bad))
    assert len(loads) + len(raises) == 3
    # what PIL still loads comes back exactly as it loads it, between sound images that stay exact
    datas = [good[0]] + [b for _, b in loads[:1]] + [good[1]] + [b for _, b in loads[1:]] + [good[2]]
    jpeg.reset_stats()
    _assert_exact(jpeg.decode_jpeg(datas), datas)
    st = jpeg.stats()
    assert st['device'] == 3 and sum(st['fallback'].values()) == len(loads) and all(k.startswith('damaged_') for k in st['fallback']), st
    # what PIL refuses raises as it does on the host path -- after the kernels have said that the stream is damaged
    for name, bad in raises:
        jpeg.reset_stats()
        with pytest.raises(OSError):
            jpeg.decode_jpeg([good[0], bad, good[1]])
        st = jpeg.stats()
        assert st['device'] == 2 and list(st['fallback'].values()) == [1] and list(st['fallback'])[0].startswith('damaged_'), (name, st)


# ---- the wiring ----------------------------------------------------------------------------------------------------------------------
def _files(tmp_path, sizes, samp=2, kind='lowpass'):
    paths = []
    for i, (h, w) in enumerate(sizes):
        paths.append(str(tmp_path / ('im%02d.jpg' % i)))
        with open(paths[-1], 'wb') as fh:
            fh.write(encode(picture(kind, h, w, seed=i), samp if i % 3 else 0, 75 + i))
    return paths


def test_cache_and_im_worker_give_the_chip_of_the_pil_cache(tmp_path, monkeypatch):
    from sniper_amd import config as cfgmod
    from sniper_amd import jpeg
    from sniper_amd.data import im_worker as iw
    monkeypatch.delenv('SNIPER_IMAGE_DECODER', raising=False)
    cfg = cfgmod.res101_e2e(batch_images=4)
    paths = _files(tmp_path, ((120, 160), (97, 131), (160, 120), (64, 64)))
    npy = str(tmp_path / 'arr.npy')
    np.save(npy, picture('noise', 20, 30))
    calls = []
    real = jpeg.decode_jpeg
    monkeypatch.setattr(jpeg, 'decode_jpeg', lambda srcs, *a, **k: calls.append(len(srcs)) or real(srcs, *a, **k))
    chips = {}
    for decoder in ('pil', 'device'):
        cache = iw.DeviceImageCache(decoder=decoder)
        crop_worker = iw.im_worker(cfg, crop_size=96, image_cache=cache)
        full_worker = iw.im_worker(cfg, target_size=(96, 128), image_cache=cache)
        iw.decode_ahead(crop_worker, paths + [npy, paths[0]], threads=4)
        assert all(cache.holds(p) for p in paths) and cache.holds(npy) and cache.misses == 5
        out = []
        for flip in (False, True):
            t = torch.zeros((3, 96, 96), dtype=torch.float32, device=dev())
            crop_worker.worker([paths[1], ((10, 5, 90, 70), 1.2), flip], t)
            out.append(t)
        t = torch.zeros((3, 96, 128), dtype=torch.float32, device=dev())
        scale, hw = full_worker.worker([paths[0], None, False], t)
        out.append(t)
        t = torch.zeros((3, 96, 128), dtype=torch.float32, device=dev())
        full_worker.worker([npy, None, False], t)
        out.append(t)
        chips[decoder] = out
        assert cache.misses == 5 and all(torch.equal(cache.get(p).cpu(), torch.from_numpy(pil_bgr(open(p, 'rb').read()))) for p in paths)
        if decoder == 'pil':
            assert calls == []
    assert calls == [4]                                          # decode_ahead filled the cache in one decode call
    for a, b in zip(chips['pil'], chips['device']):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    # a cache miss outside decode_ahead decodes on the device too, and an eviction frees the tensor's own storage
    cache = iw.DeviceImageCache(max_bytes=120 * 160 * 3 + 10, decoder='device')
    a = cache.get(paths[0])
    assert a.untyped_storage().nbytes() == a.numel() and calls == [4, 1]
    cache.get(paths[2])
    assert len(cache) == 1 and not cache.holds(paths[0])


def test_iterator_batches_are_identical_under_both_decoders(tmp_path, monkeypatch):
    from sniper_amd import config as cfgmod
    from sniper_amd import jpeg
    from sniper_amd.iterators import MNIteratorE2E
    from sniper_amd.synthetic import make_roidb
    monkeypatch.delenv('SNIPER_IMAGE_DECODER', raising=False)
    base = make_roidb(6, seed=3, n_proposals=300)
    paths = _files(tmp_path, [(r['height'], r['width']) for r in base])
    batches = {}
    for decoder in ('pil', 'device'):
        cfg = cfgmod.res101_e2e(batch_images=4)
        if decoder == 'device':
            cfg.IMAGE_DECODER = 'device'
        roidb = [dict(r, image=p) for r, p in zip(base, paths)]
        np.random.seed(3)
        jpeg.reset_stats()
        it = MNIteratorE2E(roidb, cfg, batch_size=4, nGPUs=1)
        assert it.im_worker._cache.decoder == decoder
        batches[decoder] = [it.batch.data[0].asnumpy()] + [lab.asnumpy() for lab in it.batch.label]
        assert (jpeg.stats()['device'] > 0) == (decoder == 'device'), jpeg.stats()
    for a, b in zip(batches['pil'], batches['device']):
        assert np.array_equal(a, b)
    assert float(np.abs(batches['pil'][0]).std()) > 10


def test_test_time_pass_gives_identical_detections_under_both_decoders(tmp_path, monkeypatch):
    import sniper_amd.mx as mx
    from sniper_amd import config as cfgmod
    from sniper_amd import inference, jpeg
    from sniper_amd.symbols.faster import resnet_mx_101_e2e as rn
    monkeypatch.delenv('SNIPER_IMAGE_DECODER', raising=False)
    paths = _files(tmp_path, ((120, 160), (120, 160)))

    class Imdb(object):
        num_classes, classes, name, result_path = 81, ['c%d' % i for i in range(81)], 'synthetic', None
    cache, final = {}, {}
    for decoder in ('pil', 'device'):
        cfg = cfgmod.res101_e2e_autofocus()
        cfg.TEST.SCALES = ((120, 160),)
        cfg.TEST.BATCH_IMAGES = (2,)
        cfg.TEST.VALID_RANGES = ((-1, -1),)
        cfg.TEST.DO_PRUNING = (False,)
        cfg.TEST.CHIP_HYPERPARAMS = ((-1, -1, -1),)
        cfg.TEST.MAX_PER_IMAGE = 50
        cfg.TEST.RPN_PRE_NMS_TOP_N, cfg.TEST.RPN_POST_NMS_TOP_N = 500, 100
        if decoder == 'device':
            cfg.IMAGE_DECODER = 'device'
        roidb = [{'image': p, 'width': 160, 'height': 120, 'flipped': False, 'gt_overlaps': np.zeros((1, 81), np.float32)} for p in paths]
        jpeg.reset_stats()
        final[decoder] = inference.imdb_detection_wrapper(rn.resnet_mx_101_e2e, cfg, Imdb(), roidb, [mx.gpu(0)], None, None, module_cache=cache)
        assert jpeg.stats()['device'] == (2 if decoder == 'device' else 0), jpeg.stats()
    n = 0
    for j in range(1, 81):
        for a, b in zip(final['pil'][j], final['device'][j]):
            assert np.array_equal(a, b)
            n += len(a)
    assert n > 0
