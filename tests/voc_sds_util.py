"""What the PASCAL VOC mask evaluation tests, tests/golden/make_vocsds_golden.py and tools/voc_sds_bench.py share: the hand-made and
seeded sets, the loader of tests/golden/vocsds_v1.npz, the records / all_boxes / all_masks forms of a set, and the device run at the C
ABI.  A SET is (gt, dt, K, I, M, binary_thresh) as tests/voc_sds_ref.py describes it."""
import os

import numpy as np

from coco_eval_util import Guarded
from voc_eval_util import assert_area_within_bound, assert_same_bits, recall_changes, same_bits  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vocsds_v1.npz')
GT_KEYS = ('image', 'category', 'bound', 'bits', 'pix_off')
DT_KEYS = ('image', 'category', 'raw', 'masks')
SETS = ('small', 'edges', 'seeded')
THRESHOLDS = (0.5, 0.7)


class Builder(object):
    """collects instances and detections in any order -> a set"""

    def __init__(self, K, I, M, binary_thresh):
        self.K, self.I, self.M, self.thr = K, I, M, binary_thresh
        self.gts, self.dts = [], []

    def inst(self, image, cat, x1, y1, mask):
        """an instance whose bound starts at (x1, y1) and has the mask's shape"""
        mask = np.asarray(mask) != 0
        h, w = mask.shape
        self.gts.append((image, cat, [x1, y1, x1 + w - 1, y1 + h - 1], mask))

    def det(self, image, cat, box, score, mask):
        mask = np.broadcast_to(np.asarray(mask, np.float32), (self.M, self.M))
        self.dts.append((image, cat, [float(v) for v in box] + [score], mask))

    def done(self):
        gts, dts, I = self.gts, self.dts, self.I
        gt = {'image': np.array([g[0] for g in gts], np.int32), 'category': np.array([g[1] for g in gts], np.int32),
              'bound': np.array([g[2] for g in gts], np.float64).reshape(-1, 4),
              'bits': np.concatenate([g[3].reshape(-1).astype(np.uint8) for g in gts]) if gts else np.zeros(0, np.uint8),
              'pix_off': np.concatenate([[0], np.cumsum([g[3].size for g in gts])]).astype(np.int64)}
        img, cat = np.array([d[0] for d in dts], np.int32), np.array([d[1] for d in dts], np.int32)
        o = np.argsort(cat.astype(np.int64) * I + img, kind='stable')
        dt = {'image': img[o], 'category': cat[o], 'raw': np.array([d[2] for d in dts], np.float32).reshape(-1, 5)[o],
              'masks': np.array([d[3] for d in dts], np.float32).reshape(-1, self.M, self.M)[o]}
        return gt, dt, self.K, self.I, self.M, self.thr


def small_set():
    """Drawable by hand: 8 x 8 images, 4 x 4 maps, two classes.  A box of 4 x 4 is the identity resize (scale 1: every coefficient 0)."""
    b = Builder(2, 3, 4, 0.4)
    one = np.ones((4, 4), np.float32)
    left = np.array([[1, 1, 0, 0]] * 4, np.float32)
    # image 0, class 0: a full 4 x 4 square; the exact detection (overlap 1) and a shifted one (4 / 28)
    b.inst(0, 0, 1, 1, np.ones((4, 4)))
    b.det(0, 0, [1, 1, 4, 4], 0.9, one)
    b.det(0, 0, [3, 3, 6, 6], 0.8, one)
    # image 1, class 0: an L of 7 pixels in a 4 x 4 bound; a detection that covers its left half (6 of 8 set pixels meet: 6 / 9)
    b.inst(1, 0, 0, 0, [[1, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [1, 1, 1, 1]])
    b.det(1, 0, [0, 0, 3, 3], 0.7, left)
    # image 2, class 0: no instance: a false positive between the matches
    b.det(2, 0, [2, 2, 5, 5], 0.75, one)
    # class 1: two instances in image 0, one in image 2; a detection for the second of image 0 only (3 / 4 of it) and a miss
    b.inst(0, 1, 4, 0, np.ones((2, 4)))
    b.inst(0, 1, 0, 6, np.ones((2, 8)))
    b.inst(2, 1, 0, 0, np.ones((3, 3)))
    b.det(0, 1, [0, 6, 7, 7.4], 0.6, np.array([[1, 1, 1, 0]] * 4, np.float32))
    b.det(2, 1, [5, 5, 7, 7], 0.5, one)
    return b.done()


def edges_set():
    """The edge cases, one per image where they must not meet; 4 x 4 maps (a 4 x 4 box is the identity, a 2 x 2 box the exact
    decimation); binary_thresh = 0.7, whose float32 value lies BELOW 0.7: a probability of float32(0.7) is set by the reference's
    float32 compare and not by a float64 one.  Classes: 0 matching rules, 1 shapes of boxes, 2 the threshold, 3 detections without any
    instance, 4 an instance without detections."""
    b = Builder(5, 8, 4, 0.7)
    one = np.ones((4, 4), np.float32)
    full = np.ones((4, 4))
    # image 0: overlap exactly 0.5 (the upper half of a full square: 8 / 16): tp at 0.5 under >=, fp at 0.7
    b.inst(0, 0, 0, 0, full)
    b.det(0, 0, [0, 0, 3, 3], 0.95, np.array([[1] * 4, [1] * 4, [0] * 4, [0] * 4], np.float32))
    # image 1: two squares side by side; A covers both (0.5 with each: the FIRST is its candidate), B is the first square itself and
    # finds it already detected at 0.5 -- the second square stays free; at 0.7 A fails and B takes it
    b.inst(1, 0, 0, 0, full)
    b.inst(1, 0, 4, 0, full)
    b.det(1, 0, [0, 0, 7, 3], 0.90, one)
    b.det(1, 0, [0, 0, 3, 3], 0.85, one)
    # image 2: no instance of class 0
    b.det(2, 0, [1, 1, 6, 6], 0.80, one)
    # image 3: an instance without a set pixel and an all-zero map over it: union 0 < 1, overlap 0, still the candidate; and a box
    # that is disjoint from every instance of its image
    b.inst(3, 0, 2, 2, np.zeros((3, 3)))
    b.det(3, 0, [2, 2, 4, 4], 0.70, np.zeros((4, 4), np.float32))
    b.det(3, 0, [10, 10, 12, 12], 0.65, one)
    # class 1, image 4: a 12 x 12 square with a hole; boxes of one pixel, one row, one column, the exact 2 x 2 decimation, a box at
    # negative coordinates, and halves that round to even (0.5 -> 0, 2.5 -> 2, 3.5 -> 4, 7.5 -> 8)
    ring = np.ones((12, 12))
    ring[4:8, 4:8] = 0
    b.inst(4, 1, 0, 0, ring)
    ramp = (np.arange(16, dtype=np.float32).reshape(4, 4) + 1) / 16
    b.det(4, 1, [1, 1, 1, 1], 0.91, one)
    b.det(4, 1, [0, 2, 11, 2], 0.82, ramp.T)
    b.det(4, 1, [3, 0, 3, 11], 0.73, ramp)
    b.det(4, 1, [8, 8, 9, 9], 0.64, np.array([[1, 1, 1, .5], [1, 1, .5, 1], [1, .6, 1, 1], [.6, 1, 1, 1]], np.float32))
    b.det(4, 1, [-3, -2, 2, 3], 0.55, one)
    b.det(4, 1, [0.5, 2.5, 3.5, 7.5], 0.46, ramp)
    b.det(4, 1, [-9, -9, -5, -5], 0.37, one)
    b.det(4, 1, [0, 0, 11, 11], 0.99, one)
    # class 2, image 5: the threshold.  An identity box whose map is float32(0.7) everywhere: all set in float32 (overlap 1), none in
    # float64; image 6: one float32 step below: nothing set
    at = np.float32(0.7)
    b.inst(5, 2, 0, 0, full)
    b.det(5, 2, [0, 0, 3, 3], 0.9, np.full((4, 4), at, np.float32))
    b.inst(6, 2, 0, 0, full)
    b.det(6, 2, [0, 0, 3, 3], 0.8, np.full((4, 4), np.nextafter(at, np.float32(0)), np.float32))
    # class 3: detections, no instance anywhere (rec = nan, AP 0).  class 4: an instance, no detections.
    b.det(0, 3, [0, 0, 5, 5], 0.5, one)
    b.det(7, 3, [1, 1, 2, 2], 0.4, one)
    b.inst(7, 4, 1, 1, np.ones((2, 5)))
    return b.done()


def _blob(rng, h, w):
    """a filled ellipse or rectangle with a bite taken out: every row and column of the bound need not be touched"""
    yy, xx = np.mgrid[0:h, 0:w]
    if rng.rand() < 0.6:
        m = ((yy - (h - 1) / 2.0) / (h / 2.0)) ** 2 + ((xx - (w - 1) / 2.0) / (w / 2.0)) ** 2 <= 1.0
    else:
        m = np.ones((h, w), bool)
    if rng.rand() < 0.5 and h > 3 and w > 3:
        m[:rng.randint(1, h // 2), :rng.randint(1, w // 2)] = False
    if not m.any():
        m[h // 2, w // 2] = True
    return m


def map_of(canvas, box, M, rng, noise=0.15, levels=32):
    """an (M, M) probability map for the float box: the canvas (h, w bool) sampled at the centres of the map's cells, noise added,
    quantised to 1 / levels (so that the golden file compresses and values ON a threshold occur)"""
    h, w = canvas.shape
    x1, y1, x2, y2 = box
    xs = np.round(x1 + (np.arange(M) + 0.5) * (x2 - x1 + 1) / M - 0.5).astype(int)
    ys = np.round(y1 + (np.arange(M) + 0.5) * (y2 - y1 + 1) / M - 0.5).astype(int)
    inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]           # zeros outside the canvas
    hit = canvas[np.ix_(np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1))] & inside
    v = 0.15 + 0.7 * hit.astype(np.float32) + rng.uniform(-noise, noise, (M, M))
    return (np.round(np.clip(v, 0, 1) * levels) / levels).astype(np.float32)


def seeded_set(seed, n_img, K, M, binary_thresh=0.4, max_hw=(48, 64), gt_per_img=2.0, dets_per_img=(4, 9), distinct=True, ties=8):
    """Images of at most max_hw with blobs as instances.  Detections: three quarters are an instance's bound jittered by +-s in
    position and exp(U(-s, s)) in size, s from {0.05, 0.15, 0.3}, with that instance's pixels as their map (several detections claim one
    instance); a quarter are random boxes of a random class with noise maps; boxes are floats and may leave the image.  distinct:
    scores distinct within every class, else quantised to 1 / ties."""
    rng = np.random.RandomState(seed)
    b = Builder(K, n_img, M, binary_thresh)
    for i in range(n_img):
        h, w = rng.randint(max_hw[0] * 5 // 8, max_hw[0] + 1), rng.randint(max_hw[1] * 5 // 8, max_hw[1] + 1)
        mine = []
        for _ in range(max(1, rng.poisson(gt_per_img))):
            bh, bw = rng.randint(3, h * 2 // 3), rng.randint(3, w * 2 // 3)
            y1, x1 = rng.randint(0, h - bh + 1), rng.randint(0, w - bw + 1)
            k, m = int(rng.randint(K)), _blob(rng, bh, bw)
            b.inst(i, k, x1, y1, m)
            canvas = np.zeros((h, w), bool)
            canvas[y1:y1 + bh, x1:x1 + bw] = m
            mine.append((k, [x1, y1, x1 + bw - 1, y1 + bh - 1], canvas))
        for _ in range(rng.randint(dets_per_img[0], dets_per_img[1])):
            if rng.rand() < 0.75:
                k, g, canvas = mine[rng.randint(len(mine))]
                s = (0.05, 0.15, 0.3)[rng.randint(3)]
                gw, gh = g[2] - g[0] + 1, g[3] - g[1] + 1
                x, y = g[0] + rng.uniform(-s, s) * gw, g[1] + rng.uniform(-s, s) * gh
                bw, bh = gw * np.exp(rng.uniform(-s, s)), gh * np.exp(rng.uniform(-s, s))
                box = [x, y, x + bw - 1, y + bh - 1]
                m = map_of(canvas, box, M, rng)
            else:
                k = int(rng.randint(K))
                bw, bh = rng.uniform(2, w * 0.7), rng.uniform(2, h * 0.7)
                x, y = rng.uniform(-3, w - bw + 3), rng.uniform(-3, h - bh + 3)
                box = [x, y, x + bw - 1, y + bh - 1]
                m = map_of(np.zeros((h, w), bool), box, M, rng, noise=0.5)
            b.det(i, k, box, 0.0, m)
    gt, dt, K, I, M, thr = b.done()
    for k in range(K):
        sel = np.flatnonzero(dt['category'] == k)
        if distinct:
            assert len(sel) <= 9999
            dt['raw'][sel, 4] = (rng.permutation(np.arange(1, 10000))[:len(sel)] / 10000.0).astype(np.float32)
        else:
            dt['raw'][sel, 4] = (rng.randint(1, ties + 1, len(sel)) / float(ties)).astype(np.float32)
    return gt, dt, K, I, M, thr


def make_sets():
    return {'small': small_set(), 'edges': edges_set(), 'seeded': seeded_set(7, 24, 3, 28)}


def tie_set():
    """equal scores within an image and across images (scores quantised to 1 / 8)"""
    return seeded_set(11, 10, 2, 7, dets_per_img=(6, 12), distinct=False, ties=8)


_CACHE = {}


def load_golden():
    """{set: (gt, dt, K, I, M, binary_thresh, ap)} from the committed file; ap (T,K) is what the reference's voc_eval_sds returned"""
    if not _CACHE:
        z = np.load(GOLDEN)
        for s in SETS:
            gt = {k: z['%s_in_gt_%s' % (s, k)] for k in GT_KEYS}
            dt = {k: z['%s_in_dt_%s' % (s, k)] for k in DT_KEYS}
            K, I, M = (int(v) for v in z['%s_shape' % s])
            _CACHE[s] = (gt, dt, K, I, M, float(z['%s_binary_thresh' % s]), z['%s_ap' % s])
    return _CACHE


# ---- the forms the public interface takes ---------------------------------------------------------------
def records_of(gt, I):
    """records[i] = what parse_inst returns for image i: dicts with mask (bool), mask_bound, mask_cls (1-based: 0 is the background)"""
    from voc_sds_ref import gt_mask
    out = [[] for _ in range(I)]
    for n in range(len(gt['image'])):
        out[int(gt['image'][n])].append({'mask': gt_mask(gt, n), 'mask_bound': np.array(gt['bound'][n]), 'mask_cls': int(gt['category'][n]) + 1})
    return out


def all_boxes_masks_of(dt, K, I, M):
    """a set's detections as all_boxes[class][image] = (n,5) float32 and all_masks[class][image] = (n,M,M) float32 (class 0 = background)"""
    boxes = [[np.zeros((0, 5), np.float32) for _ in range(I)] for _ in range(K + 1)]
    masks = [[np.zeros((0, M, M), np.float32) for _ in range(I)] for _ in range(K + 1)]
    key = dt['category'].astype(np.int64) * I + dt['image']
    for kk in np.unique(key):
        boxes[int(kk // I) + 1][int(kk % I)] = dt['raw'][key == kk]
        masks[int(kk // I) + 1][int(kk % I)] = dt['masks'][key == kk]
    return boxes, masks


# ---- the device, at the C ABI, with every operand in a guarded buffer ---------------------------------
OVERLAP_KEYS = ('dt_area', 'iou')
MATCH_KEYS = ('dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det')
CURVE_KEYS = ('order', 'rec', 'prec', 'npos', 'ap07', 'ap_area')
DEVICE_KEYS = OVERLAP_KEYS + MATCH_KEYS + CURVE_KEYS
EXACT_KEYS = tuple(k for k in DEVICE_KEYS if k != 'ap_area')


def limits():
    import ctypes
    from sniper_amd import hip
    out = (ctypes.c_int32 * 6)()
    hip.lib().call('sn_vocsds_limits', out)
    return list(out)


def device_run(gt, dt, K, thresholds, binary_thresh, ev):
    """sn_vocsds_mask_iou + sn_vocsds_match_iou + sn_voc_accumulate on the CSR layout `ev` (the restatement's offsets, permutation
    and rounded boxes) -> the arrays named in DEVICE_KEYS; every operand guarded, the guards checked"""
    import torch
    from sniper_amd import hip
    gp = ev['gt_perm']
    thrs = np.asarray(thresholds, np.float64)
    T, ND, NG, P = len(thrs), len(dt['image']), len(gp), len(ev['prob_cat'])
    assert P >= 1 and ND >= 1
    M = dt['masks'].shape[1]
    dcount, gcount = np.diff(ev['dt_off']), np.diff(ev['gt_off'])
    per_class = np.diff(ev['dt_off'][ev['cat_off']].astype(np.int64))
    bound = np.round(np.asarray(gt['bound'], np.float64)).astype(np.int32).reshape(-1, 4)[gp]
    sizes = np.diff(gt['pix_off'])[gp]
    bits = np.concatenate([gt['bits'][gt['pix_off'][g]:gt['pix_off'][g + 1]] for g in gp]) if NG else np.zeros(0, np.uint8)
    pix_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    area = np.array([int((gt['bits'][gt['pix_off'][g]:gt['pix_off'][g + 1]] != 0).sum()) for g in gp], np.int32)
    box = np.asarray(ev['dt_box'], np.int32)
    pixels = (box[:, 2].astype(np.int64) - box[:, 0] + 1) * (box[:, 3].astype(np.int64) - box[:, 1] + 1)
    n_pairs = int(ev['iou_off'][-1])
    G = Guarded()
    d_masks, d_box = G.put(np.ascontiguousarray(dt['masks'], np.float32)), G.put(box)
    d_score = G.put(np.asarray(dt['raw'])[:, 4].astype(np.float64))
    d_bits, d_pix, d_bound, d_area = G.put(bits), G.put(pix_off), G.put(bound), G.put(area)
    d_dt_off, d_gt_off, d_cat_off, d_iou_off = (G.put(ev[k].astype(np.int32)) for k in ('dt_off', 'gt_off', 'cat_off', 'iou_off'))
    d_thr, d_zero = G.put(thrs), G.put(np.zeros(NG, np.uint8))
    shapes = {'dt_area': ((ND,), np.int32), 'iou': ((n_pairs,), np.float64), 'dt_best': ((ND,), np.int32), 'dt_iou': ((ND,), np.float64),
              'dt_tp': ((T, ND), np.uint8), 'dt_fp': ((T, ND), np.uint8), 'gt_det': ((T, NG), np.int32), 'order': ((ND,), np.int32),
              'rec': ((T, ND), np.float64), 'prec': ((T, ND), np.float64), 'npos': ((K,), np.int32), 'ap07': ((T, K), np.float64),
              'ap_area': ((T, K), np.float64)}
    o = {k: G.out(*shapes[k]) for k in DEVICE_KEYS}
    need = int(hip.query('sn_voc_accumulate_workspace_bytes', ND, T))
    ws = G.out((need,), np.uint8)
    hip.call('sn_vocsds_mask_iou', d_masks, d_box, d_dt_off, d_bits, d_pix, d_bound, d_area, d_gt_off, d_iou_off, P, M,
             float(np.float32(binary_thresh)), int(gcount.max()), ND, NG, n_pairs, int(pixels.max()), o['dt_area'], o['iou'], hip.stream())
    hip.call('sn_vocsds_match_iou', d_score, d_dt_off, d_gt_off, o['iou'], d_iou_off, d_thr, P, T, int(dcount.max()), int(gcount.max()), ND, NG,
             o['dt_best'], o['dt_iou'], o['dt_tp'], o['dt_fp'], o['gt_det'], hip.stream())
    hip.call('sn_voc_accumulate', d_score, d_dt_off, d_gt_off, d_cat_off, d_zero, o['dt_tp'], o['dt_fp'], np.arange(0., 1.1, 0.1), P, K, T,
             int(per_class.max()), ND, NG, ws, need, o['order'], o['rec'], o['prec'], o['npos'], o['ap07'], o['ap_area'], hip.stream())
    torch.cuda.synchronize()
    G.check()
    return {k: Guarded.read(o[k], *shapes[k]) for k in DEVICE_KEYS}


def check_device(gt, dt, K, thresholds, binary_thresh, what, want=None, twice=True):
    """device == restatement on every exact key, the area AP within its bound; two runs identical -> (got, want)"""
    import voc_sds_ref as ref
    if want is None:
        want = ref.run(gt, dt, K, thresholds, binary_thresh)
    got = device_run(gt, dt, K, thresholds, binary_thresh, want)
    assert_same_bits(got, want, keys=EXACT_KEYS, what=what)
    assert_area_within_bound(got['ap_area'], want['ap_area'], recall_changes(want['rec'], want['cls_off']), what)
    if twice:
        again = device_run(gt, dt, K, thresholds, binary_thresh, want)
        for k in DEVICE_KEYS:
            assert got[k].tobytes() == again[k].tobytes(), (what, k, 'two runs differ')
    return got, want
