"""GPU: the JPEG encoder (sniper_amd/jpeg_encode.py, csrc/jpeg_encode.hip).  Every file is compared byte for byte with the file PIL
writes for the same picture and parameters; the quantised blocks are compared with the numpy restatement tests/jpeg_enc_ref.py."""
import io
import os

import numpy as np
import pytest

import jpeg_enc_ref as ref

pytestmark = pytest.mark.gpu

SUBS = ('4:2:0', '4:2:2', '4:4:4')


@pytest.fixture(scope='module')
def je():
    from sniper_amd import jpeg_encode as mod
    return mod


def _pil(pic, q=75, sub='4:2:0'):
    # (grey: the sampling is ignored here, which is PIL's file when it is told 4:4:4 or nothing)
    return ref.pil_encode(pic, q, sub if pic.ndim == 3 else '4:4:4')


def _equal(files, pics, q=75, sub='4:2:0'):
    assert len(files) == len(pics)
    bad = [(i, p.shape) for i, (f, p) in enumerate(zip(files, pics)) if f != _pil(p, q, sub)]
    assert not bad, (q, sub, bad)


# ---- the stage before coding -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub,grey', [('4:2:0', False), ('4:2:2', False), ('4:4:4', False), ('4:2:0', True)], ids=['420', '422', '444', 'grey'])
def test_coefficients_equal_the_restatement(je, sub, grey):
    sizes = ((8, 8), (17, 16), (16, 17), (24, 50), (31, 3))
    for kind, q in (('noise', 75), ('pixel_checker', 100), ('smooth', 30)):
        pics = [ref.picture(kind, h, w, grey) for h, w in sizes]
        coef, off = je.jpeg_coefficients(pics, q, sub)
        host = coef.cpu().numpy()
        assert host.dtype == np.int16 and host.shape == (off[-1], 64) and off[0] == 0
        for i, p in enumerate(pics):
            want = ref.blocks(p, q, sub)
            assert off[i + 1] - off[i] == len(want)
            assert np.array_equal(host[off[i]:off[i + 1]], want), (kind, q, sub, grey, p.shape)


# ---- whole files ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,q', [('smooth', 75), ('noise', 100), ('noise', 10), ('pixel_checker', 100), ('pixel_checker', 1),
                                    ('block_checker', 100), ('block_checker', 1), ('flat', 75)])
def test_every_size_in_one_ragged_call(je, kind, q):
    pics = [ref.picture(kind, h, w) for h, w in ref.SIZES] + [ref.picture(kind, h, w, grey=True) for h, w in ref.SIZES]
    _equal(je.encode_jpeg(pics, q), pics, q)


@pytest.mark.parametrize('sub', ['4:2:2', '4:4:4'])
def test_the_other_samplings(je, sub):
    for kind, q in (('smooth', 75), ('noise', 100), ('block_checker', 1)):
        pics = [ref.picture(kind, h, w) for h, w in ref.SIZES]
        _equal(je.encode_jpeg(pics, q, sub), pics, q, sub)


def test_numpy_arrays_device_tensors_and_a_second_call_give_the_same_bytes(je):
    import torch
    pics = [ref.picture('noise', h, w, seed=3) for h, w in ((33, 40), (1, 1), (67, 101), (16, 17))] + [ref.picture('smooth', 25, 7, grey=True)]
    a = je.encode_jpeg(pics, 90)
    dev = [torch.as_tensor(p).cuda() for p in pics]
    b = je.encode_jpeg(dev, 90)
    mixed = je.encode_jpeg([dev[0], pics[1], dev[2], pics[3], dev[4]], 90)
    assert a == b == mixed == je.encode_jpeg(pics, 90)
    _equal(a, pics, 90)


def test_nothing_is_written_behind_the_declared_capacity(je):
    pics = [ref.picture('pixel_checker', 67, 101), ref.picture('noise', 48, 64), ref.picture('noise', 3, 5, grey=True)]
    _equal(je.encode_jpeg(pics, 100, '4:4:4', _guard=4096), pics, 100, '4:4:4')          # (raises when the pattern is touched)


def test_one_pixel_alone(je):
    for pic in (np.array([[[7, 200, 31]]], np.uint8), np.array([[255]], np.uint8), np.array([[[255, 255, 255]]], np.uint8)):
        for sub in SUBS:
            _equal(je.encode_jpeg([pic], 75, sub), [pic], 75, sub)


def test_a_scan_that_spans_several_workgroups_of_every_kernel(je):
    lim = je.jpeg_enc_limits()
    threads, chunk = lim['threads'], lim['chunk']
    # the smallest odd-sized noise picture (quality 100, 4:4:4) with more than two workgroups of blocks (a lane per block) and more
    # than two workgroups of raw chunks (a lane per `chunk` bytes of the unstuffed scan)
    found = None
    for side in range(11, 600, 8):
        pic = ref.picture('noise', side, side + 2)
        blocks = 3 * -(-side // 8) * -(-(side + 2) // 8)
        if blocks <= 2 * threads:
            continue
        want = ref.pil_encode(pic, 100, '4:4:4')
        scan = want[len(je.jpeg_header(side, side + 2, 100, '4:4:4')):-2]
        if len(scan.replace(b'\xff\x00', b'\xff')) > 2 * threads * chunk:
            found = (pic, want)
            break
    assert found is not None and found[0].shape[0] <= 160, 'the size is derived from the limits: %r' % (lim,)
    pic, want = found
    small = ref.picture('smooth', 9, 23)
    files = je.encode_jpeg([small, pic, small], 100, '4:4:4')
    assert files[1] == want and files[0] == files[2] == ref.pil_encode(small, 100, '4:4:4')
    # and 4:2:0, where an MCU is six blocks and the workgroup borders fall inside MCUs
    assert je.encode_jpeg([pic], 100)[0] == ref.pil_encode(pic, 100)


def test_the_projects_decoder_reads_the_projects_files(je):
    from PIL import Image
    from sniper_amd import jpeg
    pics = [ref.picture('smooth', 33, 40), ref.picture('noise', 67, 101), ref.picture('noise', 16, 17)]
    for sub in SUBS:
        files = je.encode_jpeg(pics, 85, sub)
        before = jpeg.stats()['device']
        got = jpeg.decode_jpeg(files)
        assert jpeg.stats()['device'] == before + len(pics)          # decoded on the device, not by the fallback
        for g, p in zip(got, pics):
            want = np.asarray(Image.open(io.BytesIO(ref.pil_encode(p, 85, sub))).convert('RGB'))[:, :, ::-1]
            assert np.array_equal(g.cpu().numpy(), want), (sub, p.shape)


# ---- the wiring --------------------------------------------------------------------------------------------------------------------------
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


def _read(path):
    with open(path, 'rb') as fh:
        return fh.read()


def test_render_results_device_encoder_writes_the_files_pil_writes(je, tmp_path):
    from sniper_amd.visualization import render_results
    roidb, boxes = _roidb(tmp_path)
    names = ['__background__', 'cat', 'dog']
    for ext in ('.jpg', '.JPEG'):
        a = render_results(roidb, boxes, names, str(tmp_path / ('pil' + ext)), vis_ext=ext)
        before = je.stats()
        b = render_results(roidb, boxes, names, str(tmp_path / ('dev' + ext)), vis_ext=ext, encoder='device')
        after = je.stats()
        assert len(a) == len(b) == 3 and after['files'] == before['files'] + 3          # (not through PIL)
        assert [os.path.basename(p) for p in a] == [os.path.basename(p) for p in b]
        assert [_read(p) for p in a] == [_read(p) for p in b]
        assert after['bytes'] == before['bytes'] + sum(len(_read(p)) for p in b)
    # another extension still goes through PIL, and the default encoder never comes here
    before = je.stats()
    c = render_results(roidb, boxes, names, str(tmp_path / 'pil_bmp'), vis_ext='.bmp')
    d = render_results(roidb, boxes, names, str(tmp_path / 'dev_bmp'), vis_ext='.bmp', encoder='device')
    render_results(roidb, boxes, names, str(tmp_path / 'pil_again'), vis_ext='.jpg', encoder='pil')
    assert [_read(p) for p in c] == [_read(p) for p in d] and je.stats() == before


def test_visualize_dets_device_encoder(je, tmp_path):
    from sniper_amd.visualization import visualize_dets
    rng = np.random.default_rng(16)
    im = rng.integers(0, 256, (50, 80, 3)).astype(np.uint8)
    dets = [[], np.array([[4, 5, 60, 40, 0.8]], np.float32)]
    p1, p2 = str(tmp_path / 'a.jpg'), str(tmp_path / 'x.jpg')
    pic1 = visualize_dets(im, dets, 1.0, None, ['bg', 'thing'], save_path=p1, transform=False)
    before = je.stats()['files']
    pic2 = visualize_dets(im, dets, 1.0, None, ['bg', 'thing'], save_path=p2, transform=False, encoder='device')
    assert je.stats()['files'] == before + 1
    assert np.array_equal(pic1, pic2) and _read(p1) == _read(p2) == _pil(pic1)


def test_tester_aggregate_vis_encoder_from_config(je, tmp_path):
    """Tester.aggregate(vis=True, vis_ext='.jpg') reads cfg.TEST.VIS_ENCODER: a 'device' run writes the files of the default run"""
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    rs = np.random.RandomState(21)
    roidb, _ = _roidb(tmp_path, 2)
    NC = 3
    d = inference._Detections([[[] for _ in roidb] for _ in range(NC)])
    for i, e in enumerate(roidb):
        for j in range(1, NC):
            xy = rs.uniform(0, [e['width'] - 30, e['height'] - 25], (3, 2))
            wh = rs.uniform(8, 30, (3, 2))
            sc = rs.uniform(0.3, 1.0, (3, 1))
            d[j][i] = [np.hstack((xy, xy + wh, sc)).astype(np.float64)]

    class Imdb(object):
        num_classes, classes, name, result_path = NC, ['__background__', 'cat', 'dog'], 'synthetic', None
    files, counted = {}, {}
    for encoder in (None, 'pil', 'device'):
        cfg = cfgmod.res101_e2e_autofocus()
        cfg.TEST.VALID_RANGES = ((-1, -1),)
        cfg.TEST.MAX_PER_IMAGE = 100
        if encoder is not None:
            cfg.TEST.VIS_ENCODER = encoder
        tester = inference.Tester(None, Imdb(), roidb, None, cfg=cfg, batch_size=1)
        out = os.path.join(str(tmp_path), 'vis_%s' % encoder)
        before = je.stats()['files']
        tester.aggregate([d], vis=True, cache_name=None, vis_path=out, vis_ext='.jpg')
        counted[encoder] = je.stats()['files'] - before
        files[encoder] = [_read(os.path.join(out, '%d.jpg' % i)) for i in range(len(roidb))]
    assert counted == {None: 0, 'pil': 0, 'device': len(roidb)}
    assert files[None] == files['pil'] == files['device']
    assert all(f[:2] == b'\xff\xd8' and f[-2:] == b'\xff\xd9' for f in files['device'])
