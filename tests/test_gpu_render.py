"""GPU: sn_render_dets (csrc/render.hip) against the numpy restatement tests/render_ref.py, byte for byte: image and tile edges, layer
order, labels, masks (the bits of the results files), culling rounds, ragged batches, the network-input form, and the wiring of
Tester.aggregate(vis=True) and render_results.  A seeded random atlas of 8 glyphs, 7 rows by 5 columns: no test depends on a font."""
import os

import numpy as np
import pytest
import torch

import render_ref as ref

pytestmark = pytest.mark.gpu

G, GH, GW = 8, 7, 5
ATLAS = np.random.RandomState(26).randint(0, 256, (G, GH, GW)).astype(np.uint8)
ATLAS[0, 0, 0], ATLAS[G - 1, GH - 1, GW - 1], ATLAS[1, 1, 1], ATLAS[1, 2, 2] = 255, 0, 128, 127


def _limits():
    from sniper_amd import visualization as V
    return V._limits()


def _image(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _items(rects, texts=None, seed=0, mask_idx=None, masks=None):
    n = len(rects)
    colors = np.random.RandomState(1000 + seed).randint(0, 255, (n, 3)).astype(np.uint8)
    return {'rects': np.array(rects, np.int32).reshape(-1, 4), 'colors': colors, 'text': [np.array(t, np.int32) for t in (texts or [[]] * n)],
            'mask_idx': np.array(mask_idx if mask_idx is not None else [-1] * n, np.int32), 'masks': masks}


def _render(images, lists, **kw):
    from sniper_amd import visualization as V
    kw.setdefault('atlas', ATLAS)
    return V.render_lists(images, lists, **kw)


def _check(images, lists, **kw):
    got = _render(images, lists, **kw)
    rk = {k: v for k, v in kw.items() if k in ('mask_alpha', 'line_width')}
    if 'binary_thresh' in kw:
        rk['thr'] = kw['binary_thresh']
    assert len(got) == len(images)
    for i, (g, im, l) in enumerate(zip(got, images, lists)):
        want = ref.render(im, l, kw.get('atlas', ATLAS), **rk)
        assert g.dtype == np.uint8 and g.shape == want.shape
        bad = np.argwhere((g != want).any(axis=2))
        assert len(bad) == 0, (i, len(bad), bad[:5].tolist(), g[tuple(bad[0])].tolist(), want[tuple(bad[0])].tolist())
    return got


def test_image_and_tile_edges():
    lim = _limits()
    tw, th = lim['tile_w'], lim['tile_h']
    h, w = 2 * th + 1, 2 * tw + 1                   # one pixel wider and one taller than a whole number of tiles
    rects = [[-30, 5, -2, 20], [w, 5, w + 40, 20], [10, -30, 40, -1], [10, h, 40, h + 9],          # wholly outside, each side
             [-5, 3, 6, 12], [w - 4, 8, w + 6, 19], [70, -4, 90, 5], [30, h - 5, 60, h + 5],           # cut by each edge
             [50, 10, 50, 10], [100, 3, 104, 30], [3, 20, 40, 23],                                  # 1 x 1; thinner than 2 * 3, both axes
             [-(1 << 30), -(1 << 30), (1 << 30), (1 << 30)]]                                          # everything inside its core
    for e in (-1, 0, 1):                            # edges on, one before and one after a tile boundary, both axes
        rects += [[tw + e, 1, tw + e + 9, 9], [tw - 12, 2, tw + e, 11], [5, th + e, 17, th + e + 8], [20, th - 9, 33, th + e],
                  [tw + e, th + e, 2 * tw + e, 2 * th + e]]
    texts = [[i % G, (i + 3) % G] if i % 3 == 0 else [] for i in range(len(rects))]
    _check([_image(h, w, 1)], [_items(rects, texts, 1)])
    _check([_image(1, 1, 2)], [_items([[0, 0, 0, 0], [-3, -3, 3, 3]], [[1], []], 2)])
    _check([_image(1, 1, 2)], [_items([], [], 2)])
    _check([_image(h, w, 1)], [_items(rects, texts, 1)], line_width=1)
    _check([_image(h, w, 1)], [_items(rects, texts, 1)], line_width=40)


def test_layer_and_item_order():
    rects = [[10, 20, 60, 50], [30, 25, 90, 45], [30, 25, 90, 45], [12, 22, 58, 48], [5, 30, 100, 60], [28, 33, 70, 70]]
    texts = [[1, 2, 3], [4], [5, 6], [], [7, 0, 1, 2], [3, 3]]            # item 5's label lies on item 4's outline and item 0's mask
    masks = np.random.RandomState(5).rand(2, 14, 14).astype(np.float32)
    lists = _items(rects, texts, 3, mask_idx=[0, -1, -1, -1, 1, -1], masks=masks)
    _check([_image(75, 110, 3)], [lists])
    a = lists['colors'].copy()
    lists['colors'][1], lists['colors'][2] = a[2], a[1]                 # identical rects: the later colour shows
    got = _check([_image(75, 110, 3)], [lists])[0]
    assert got[25, 50].tolist() == a[1].tolist()


def test_labels():
    h, w = 40, 90
    rects = [[5, 20, 30, 35],                        # above the box
             [40, 3, 60, 30],                        # flipped inside at the image top (3 - 9 < 0)
             [40, 9, 50, 12],                        # top exactly at 0: still above
             [70, 25, 88, 38],                       # cut by the right edge
             [10, 39, 30, 60],                       # cut by the bottom edge (its top is 30)
             [60, 33, 63, 36],                       # a text wider than its box, running out of the image
             [2, 12, 9, 14]]                         # no text
    texts = [[0, G - 1], [G - 1, 0, 3], [2], [1, 2, 3, 4, 5, 6], [7, 7, 7], [0, 1, 2, 3, 4, 5, 6, 7, 0, 1], []]
    _check([_image(h, w, 4)], [_items(rects, texts, 4)])
    no_labels = _check([_image(h, w, 4)], [_items(rects, texts, 4)], atlas=None)[0]
    empty = _check([_image(h, w, 4)], [_items(rects, None, 4)])[0]
    assert np.array_equal(no_labels, empty)


def _rle_bitmap(cnts, h, w):
    return np.repeat(np.arange(len(cnts)) & 1, np.asarray(cnts, np.int64)).astype(bool).reshape(w, h).T


@pytest.mark.parametrize('M', [1, 14, 28])
def test_masks_are_the_bits_of_the_results_files(M):
    from sniper_amd import evaluation
    rs = np.random.RandomState(M)
    h, w = 37, 83
    rects = [[3, 2, 40, 30], [50, 5, 50, 36], [0, 0, w - 1, h - 1], [60, 10, 73, 23], [20, 20, 21, 21]]          # a column; the image; 14 x 14
    if M == 28:
        assert rects[3][2] - rects[3][0] + 1 == 14                     # the exact 2 x 2 area branch of the paste
    masks = rs.rand(len(rects), M, M).astype(np.float32)
    masks[2] = 0.25 + 0.5 * (rs.rand(M, M) > 0.3)
    lists = _items(rects, [[1, 2], [], [3], [], [4]], M, mask_idx=list(range(len(rects))), masks=masks)
    _check([_image(h, w, M)], [lists])
    _check([_image(h, w, M)], [lists], mask_alpha=0, binary_thresh=0.55)
    # a white image, alpha 256, black, nothing else drawn over the mask: its black pixels are the decoded paste of the same detection
    rles = evaluation.rle_paste(masks, np.array(rects), np.tile([[h, w]], (len(rects), 1)), 0.4)
    for k, rect in enumerate(rects):
        one = {'rects': np.array([rect], np.int32), 'colors': np.zeros((1, 3), np.uint8), 'text': [[]], 'mask_idx': np.array([0], np.int32),
               'masks': masks[k:k + 1]}
        pic = _render([np.full((h, w, 3), 255, np.uint8)], [one], mask_alpha=256, line_width=1)[0]
        black = (pic == 0).all(axis=2)
        x1, y1, x2, y2 = rect
        core = np.zeros((h, w), bool)
        core[y1 + 1:y2, x1 + 1:x2] = True              # (off the outline, which is black too)
        bits = _rle_bitmap(rles[k], h, w)
        border = np.zeros((h, w), bool)
        border[y1:y2 + 1, x1:x2 + 1] = True
        border &= ~core
        assert np.array_equal(black & core, bits & core) and np.array_equal(black, bits | border) and ((pic == 255).all(axis=2) | black).all()
    with pytest.raises(ValueError):
        _render([_image(h, w, M)], [_items([[3, 2, w, 30]], None, 0, mask_idx=[0], masks=masks[:1])])          # no paste box


def test_culling_rounds_and_the_item_cap():
    lim = _limits()
    tw, th, per_round, cap = lim['tile_w'], lim['tile_h'], lim['round'], lim['max_items']
    rs = np.random.RandomState(8)
    h, w = 3 * th, 3 * tw
    # more items in tile (0, 0) than a round holds, labels among them, masks too: the layer order must hold across rounds
    n = per_round + 77
    xy = np.stack([rs.randint(-4, tw - 8, n), rs.randint(-4, th - 4, n)], 1)
    rects = np.hstack([xy, xy + rs.randint(0, 12, (n, 2))])
    texts = [[int(k) % G] if k % 5 == 0 else [] for k in range(n)]
    masks = rs.rand(4, 14, 14).astype(np.float32)
    mask_idx = -np.ones(n, np.int64)
    for q, k in enumerate((3, per_round - 1, per_round, n - 1)):
        rects[k] = [2 + q, 1, 30 + q, 12]
        mask_idx[k] = q
    img = _image(h, w, 8)
    got = _check([img], [_items(rects, texts, 8, mask_idx=mask_idx, masks=masks)])[0]
    assert np.array_equal(got[2 * th:, 2 * tw:], img[2 * th:, 2 * tw:])            # a tile every item misses equals the source
    assert np.array_equal(got[:, 2 * tw:], img[:, 2 * tw:])
    # exactly the cap, spread over the image, every round partly culled
    xy = np.stack([rs.randint(-10, w, cap), rs.randint(-10, h - th, cap)], 1)
    rects = np.hstack([xy, xy + rs.randint(0, 30, (cap, 2))])
    rects[:, 3] = np.minimum(rects[:, 3], h - th - 1)
    texts = [[int(k) % G, 1] if k % 97 == 0 and rects[k, 1] > GH + 2 else [] for k in range(cap)]
    got = _check([img], [_items(rects, texts, 9)])[0]
    assert np.array_equal(got[h - th:], img[h - th:])
    with pytest.raises(ValueError):
        _render([img], [_items(np.vstack([rects, rects[:1]]), None, 9)])


def test_ragged_batch_with_an_empty_image():
    ims = [_image(21, 70, 10), _image(33, 17, 11), _image(5, 131, 12)]
    lists = [_items([[3, 3, 60, 18], [62, 0, 80, 30]], [[1, 2], [3]], 10), _items([], [], 11),
             _items([[100, -2, 129, 3], [0, 0, 130, 4]], [[], [5, 6, 7]], 12)]
    got = _check(ims, lists)
    assert np.array_equal(got[1], ims[1])
    dev_got = _render([torch.from_numpy(i).cuda() for i in ims], lists)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), g) for t, g in zip(dev_got, got))


def test_tensor_form_clamps_and_truncates():
    rs = np.random.RandomState(13)
    x = rs.uniform(-200, 200, (2, 3, 9, 70)).astype(np.float32)
    x[0, :, 0, :8] = np.array([-300.7, -0.9, 0.9, 1.0, 254.99, 255.0, 300.0, 77.5], np.float32) - 100
    means = (103.06, 115.9, 123.15)
    lists = [_items([[2, 2, 40, 7], [60, -3, 75, 5]], [[1], [2, 3]], 13), _items([[0, 0, 69, 8]], [[4, 5]], 14)]
    src = [ref.from_tensor(x[b], means) for b in range(2)]
    assert src[0].min() == 0 and src[0].max() == 255 and 0 < np.mean(src[0] == 0) < 0.5
    from sniper_amd import visualization as V
    for source in (x, torch.from_numpy(x).cuda()):
        got = V.render_lists(source, lists, atlas=ATLAS, means=means)
        for b in range(2):
            g = got[b].cpu().numpy() if isinstance(got[b], torch.Tensor) else got[b]
            assert g.shape == (9, 70, 3) and np.array_equal(g, ref.render(src[b], lists[b], ATLAS))
    plain = V.render_lists(x, [_items([], [], 0)] * 2, atlas=ATLAS, means=means)
    assert np.array_equal(plain[0], src[0]) and np.array_equal(plain[1], src[1])


def test_two_runs_give_the_same_bytes():
    rs = np.random.RandomState(15)
    n = 300
    xy = np.stack([rs.randint(-10, 150, n), rs.randint(-10, 60, n)], 1)
    rects = np.hstack([xy, xy + rs.randint(0, 50, (n, 2))])
    lists = [_items(rects, [[int(k) % G] * (k % 4) for k in range(n)], 15)]
    img = [_image(70, 160, 15)]
    a, b = _render(img, lists)[0], _render(img, lists)[0]
    assert np.array_equal(a, b) and not np.array_equal(a, img[0])


def _roidb(tmp_path, sizes):
    from PIL import Image
    roidb = []
    for i, (h, w) in enumerate(sizes):
        path = os.path.join(str(tmp_path), 'im%d.png' % i)
        Image.fromarray(_image(h, w, 20 + i)).save(path)
        roidb.append({'image': path, 'height': h, 'width': w, 'flipped': False})
    return roidb


def _ref_picture(entry, dets, names, masks=None):
    from PIL import Image
    from sniper_amd import visualization as V
    im = np.asarray(Image.open(entry['image']).convert('RGB'))
    L = V.draw_list(dets, 1.0, names, 0.5, masks, im.shape[:2])
    atlas = V.default_atlas()
    L['text'] = [V.encode_text(s) for s in L['labels']]
    return ref.render(im, L, atlas), L


def test_aggregate_vis_writes_the_picture_of_the_boxes_it_returns(tmp_path):
    """Tester(None, db_info, roidb, None, cfg=...).aggregate(dets, vis=True, vis_path=..., vis_name='x', vis_ext='.png'), as demo.py
    calls it: the file's pixels are the restatement's on the returned boxes, and the boxes are those of vis=False."""
    from PIL import Image
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    rs = np.random.RandomState(21)
    NC, sizes = 4, [(60, 90), (48, 70)]
    roidb = _roidb(tmp_path, sizes)
    cfg = cfgmod.res101_e2e_autofocus()
    cfg.TEST.VALID_RANGES = ((-1, -1), (-1, -1))
    cfg.TEST.MAX_PER_IMAGE = 100

    def scale_dets():
        out = []
        for s_i in range(2):
            d = inference._Detections([[[] for _ in sizes] for _ in range(NC)])
            for i, (h, w) in enumerate(sizes):
                for j in range(1, NC):
                    n = 3
                    xy = rs.uniform(0, [w - 30, h - 25], (n, 2))
                    wh = rs.uniform(8, 30, (n, 2))
                    sc = rs.uniform(0.3, 1.0, (n, 1))
                    d[j][i] = [np.hstack((xy, xy + wh, sc)).astype(np.float64)]
            out.append(d)
        return out

    class Imdb(object):
        num_classes, classes, name, result_path = NC, ['__background__', 'ant', 'bee', 'cow'], 'synthetic', None
    dets = scale_dets()
    tester = inference.Tester(None, Imdb(), roidb, None, cfg=cfg, batch_size=1)
    plain = tester.aggregate(dets, vis=False, cache_name=None)
    out_dir = os.path.join(str(tmp_path), 'vis')
    got = tester.aggregate(dets, vis=True, cache_name=None, vis_path=out_dir, vis_name='x', vis_ext='.png')
    for j in range(1, NC):
        for i in range(len(sizes)):
            assert np.array_equal(np.asarray(got[j][i]), np.asarray(plain[j][i]))
    assert os.listdir(out_dir) == ['x.png']                              # (one name for every image, as in the reference: the last one stays)
    last = len(sizes) - 1
    want, L = _ref_picture(roidb[last], [[]] + [got[j][last] for j in range(1, NC)], Imdb.classes)
    assert len(L['rects']) >= 2 and not np.array_equal(want, np.asarray(Image.open(roidb[last]['image'])))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, 'x.png')).convert('RGB')), want)
    # without a name: one file per image, by its index
    each = os.path.join(str(tmp_path), 'each')
    tester.aggregate(dets, vis=True, cache_name=None, vis_path=each, vis_ext='.png')
    assert sorted(os.listdir(each)) == ['0.png', '1.png']
    for i in range(len(sizes)):
        want, _ = _ref_picture(roidb[i], [[]] + [got[j][i] for j in range(1, NC)], Imdb.classes)
        assert np.array_equal(np.asarray(Image.open(os.path.join(each, '%d.png' % i)).convert('RGB')), want)


def test_chips_are_drawn_from_the_batch_tensor(tmp_path):
    """what get_detections(vis=True) and extract_proposals(vis=True) do with a batch: the `data` tensor in HBM, the means of
    transform_im (PIXEL_MEANS[[2, 1, 0]]), scale im_info[i, 2], one file per chip"""
    from PIL import Image
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    from sniper_amd import visualization as V
    rs = np.random.RandomState(23)
    cfg = cfgmod.res101_e2e_autofocus()
    x = rs.uniform(-140, 160, (2, 3, 40, 72)).astype(np.float32)
    info = np.array([[40, 72, 0.5], [40, 72, 1.25]], np.float32)

    class Arr(object):
        def __init__(self, a, device=False):
            self._data = torch.from_numpy(a).cuda() if device else a

        def asnumpy(self):
            return self._data.cpu().numpy() if isinstance(self._data, torch.Tensor) else self._data

    class Imdb(object):
        num_classes, classes, name, result_path = 3, ['__background__', 'ant', 'bee'], 'synthetic', None
    dets = [[[], np.array([[10, 20, 90, 60, 0.9], [3, 3, 11, 11, 0.4]], np.float32), np.array([[41, 5, 99, 33, 0.5]], np.float32)],
            [[], np.zeros((0, 5), np.float32), np.array([[8.4, 2.2, 40.6, 25, 0.75]], np.float32)]]
    tester = inference.Tester(None, Imdb(), [{}, {}], None, cfg=cfg, batch_size=2)
    means = np.asarray(cfg.network.PIXEL_MEANS, np.float32)[[2, 1, 0]]
    for device in (True, False):
        out_dir = os.path.join(str(tmp_path), 'chips%d' % device)
        tester._vis_chips({'data': Arr(x, device), 'im_info': Arr(info)}, lambda i: dets[i], lambda i: '7_%d' % i, Imdb.classes, out_dir, '.png')
        assert sorted(os.listdir(out_dir)) == ['7_0.png', '7_1.png']
        for i in range(2):
            L = V.draw_list(dets[i], float(info[i, 2]), Imdb.classes)
            L['text'] = [V.encode_text(s) for s in L['labels']]
            want = ref.render(ref.from_tensor(x[i], means), L, V.default_atlas())
            assert len(L['rects']) == (2, 1)[i]
            assert np.array_equal(np.asarray(Image.open(os.path.join(out_dir, '7_%d.png' % i)).convert('RGB')), want)


def test_render_results_with_masks(tmp_path):
    from PIL import Image
    from sniper_amd import visualization as V
    rs = np.random.RandomState(22)
    sizes, NC, names = [(50, 64), (33, 80)], 3, ['__background__', 'ant', 'bee']
    roidb = _roidb(tmp_path, sizes)
    all_boxes = [[[] for _ in sizes] for _ in range(NC)]
    all_masks = [[np.zeros((0, 28, 28), np.float32) for _ in sizes] for _ in range(NC)]
    for i, (h, w) in enumerate(sizes):
        for j in range(1, NC):
            n = 0 if (i, j) == (1, 1) else 3
            xy = rs.uniform(-5, [w - 20, h - 15], (n, 2))
            all_boxes[j][i] = np.hstack((xy, xy + rs.uniform(6, 40, (n, 2)), rs.uniform(0.2, 1.0, (n, 1)))).astype(np.float32)
            all_masks[j][i] = rs.rand(n, 28, 28).astype(np.float32)
    out_dir = os.path.join(str(tmp_path), 'masks')
    paths = V.render_results(roidb, all_boxes, names, out_dir, all_masks=all_masks, budget_bytes=1)          # (a batch per image)
    assert [os.path.basename(p) for p in paths] == ['0.png', '1.png']
    for i in range(len(sizes)):
        want, L = _ref_picture(roidb[i], [[]] + [all_boxes[j][i] for j in range(1, NC)], names, [None] + [all_masks[j][i] for j in range(1, NC)])
        assert (L['mask_idx'] >= 0).all() and len(L['rects']) >= 1
        assert np.array_equal(np.asarray(Image.open(paths[i]).convert('RGB')), want)
    one = V.render_results(roidb, all_boxes, names, os.path.join(str(tmp_path), 'one'), all_masks=all_masks)      # (one batch)
    for a, b in zip(paths, one):
        assert np.array_equal(np.asarray(Image.open(a)), np.asarray(Image.open(b)))
