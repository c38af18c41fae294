"""What the PASCAL VOC evaluation tests and tests/golden/make_voceval_golden.py share: the seeded generator of annotations and
detections, the hand-made edge problems, the loader of tests/golden/voceval_v1.npz, and the device run at the C ABI.

A SET is (gt, dt, K, I):
  gt = dict(image, category, bbox (n,4) x1, y1, x2, y2 integer-valued and 1-based as the XML holds them, difficult), annotation order;
  dt = dict(image, category, raw (n,5) float32 rows x1, y1, x2, y2, score as the test run holds them (0-based)), sorted class-major,
       image, row -- the order of the reference's result files.
The ROWS of a set are what write_pascal_results writes and voc_eval reads back: (n,5) float64, x + 1 to one decimal, the score to
three.  In the golden sets the scores of a class are distinct AFTER that rounding: the reference's order of equal scores is
undefined (np.argsort(-confidence) is not stable), so only such inputs have a reference answer."""
import os

import numpy as np

from coco_eval_util import Guarded

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'voceval_v1.npz')
GT_KEYS = ('image', 'category', 'bbox', 'difficult')
DT_KEYS = ('image', 'category', 'raw')
GOLDEN_KEYS = ('rows', 'cls_off', 'rec', 'prec', 'ap07', 'ap_area')
SETS = ('small', 'edges', 'voc_like')
THRESHOLDS = (0.5, 0.7)


def pack_gt(rows):
    return {'image': np.array([r[0] for r in rows], np.int32), 'category': np.array([r[1] for r in rows], np.int32),
            'bbox': np.array([r[2] for r in rows], np.float64).reshape(-1, 4), 'difficult': np.array([r[3] for r in rows], np.int32)}


def pack_dt(rows, I):
    """(image, category, [x1, y1, x2, y2, score]) in any order -> dt, sorted class-major, image, arrival"""
    img = np.array([r[0] for r in rows], np.int32)
    cat = np.array([r[1] for r in rows], np.int32)
    raw = np.array([r[2] for r in rows], np.float32).reshape(-1, 5)
    o = np.argsort(cat.astype(np.int64) * I + img, kind='stable')
    return {'image': img[o], 'category': cat[o], 'raw': raw[o]}


def result_rows(raw):
    """the rows of the result file, the slow way: the format strings of write_pascal_results read back with float()"""
    out = np.empty((len(raw), 5), np.float64)
    for n, r in enumerate(raw):
        out[n, :4] = [float('{:.1f}'.format(r[c] + 1)) for c in range(4)]
        out[n, 4] = float('{:.3f}'.format(r[4]))
    return out


def _distinct_scores(rng, n):
    """n scores whose 3-decimal roundings are distinct: k / 1000 + a jitter below 0.0004, k a sample of 1 .. 999 without repeats"""
    assert n <= 999
    k = rng.permutation(np.arange(1, 1000))[:n]
    return (k / 1000.0 + rng.uniform(-0.0004, 0.0004, n)).astype(np.float32)


def seeded_set(seed, n_img, n_cat, gt_per_img, dets_per_img, distinct=True, ties=50):
    """Boxes of 8..300 pixels at integer 1-based coordinates, 15 % difficult.  Detections: three quarters are copies of a box of
    their image jittered by +-s*w, +-s*h in position and exp(U(-s, s)) in size with s from {0.03, 0.08, 0.2} (several detections
    claim one box), a quarter random boxes of a random class; dets_per_img(i, rng) of them in image i.  distinct: scores whose
    roundings are distinct within every class; else scores quantised to 1 / ties."""
    rng = np.random.RandomState(seed)
    gts, dts = [], []
    for i in range(n_img):
        mine = []
        for _ in range(max(1, rng.poisson(gt_per_img))):
            w, h = np.exp(rng.uniform(np.log(8), np.log(300), 2))
            x, y = rng.uniform(1, 500, 2)
            b = [int(x), int(y), int(x + w), int(y + h)]
            k = int(rng.randint(n_cat))
            gts.append((i, k, b, int(rng.rand() < 0.15)))
            mine.append((k, b))
        for _ in range(dets_per_img(i, rng)):
            if rng.rand() < 0.75:
                k, b = mine[rng.randint(len(mine))]
                s = (0.03, 0.08, 0.2)[rng.randint(3)]
                w, h = b[2] - b[0] + 1, b[3] - b[1] + 1
                x = b[0] - 1 + rng.uniform(-s, s) * w
                y = b[1] - 1 + rng.uniform(-s, s) * h
                w, h = w * np.exp(rng.uniform(-s, s)), h * np.exp(rng.uniform(-s, s))
            else:
                k = int(rng.randint(n_cat))
                w, h = np.exp(rng.uniform(np.log(8), np.log(300), 2))
                x, y = rng.uniform(0, 500, 2)
            dts.append((i, k, [x, y, x + w - 1, y + h - 1, 0.0]))
    gt, dt = pack_gt(gts), pack_dt(dts, n_img)
    for k in range(n_cat):
        sel = np.flatnonzero(dt['category'] == k)
        if distinct:
            dt['raw'][sel, 4] = _distinct_scores(rng, len(sel))
        else:
            dt['raw'][sel, 4] = (rng.randint(1, ties + 1, len(sel)) / float(ties)).astype(np.float32)
    return gt, dt, n_cat, n_img


def edges_set():
    """The hand-made problems, one case per image; six classes: 0 the IoU and matching cases, 1 rounding, 2 no detections,
    3 detections and only difficult boxes (npos = 0), 4 neither, 5 detections without any box."""
    gts, dts = [], []
    G = lambda i, k, b, diff=0: gts.append((i, k, [float(v) for v in b], diff))
    # a detection given in the result file's 1-based coordinates: the raw row is one less
    D = lambda i, k, b, s: dts.append((i, k, [b[0] - 1., b[1] - 1., b[2] - 1., b[3] - 1., s]))
    # 0, 1: IoU exactly 0.5 and exactly 0.7 (a 10 x 10 box, a 10 x 5 and a 10 x 7 detection inside it): `>` leaves both unmatched at
    # their own threshold, and the second detection (IoU 0.9) then takes the box
    G(0, 0, [1, 1, 10, 10]); D(0, 0, [1, 1, 10, 5], 0.95); D(0, 0, [1, 1, 10, 9], 0.40)
    G(1, 0, [1, 1, 10, 10]); D(1, 0, [1, 1, 10, 7], 0.94); D(1, 0, [1, 1, 10, 9], 0.41)
    # 2: two identical boxes -- argmax names the first, so the second detection is a false positive and the second box stays free
    G(2, 0, [20, 20, 60, 70]); G(2, 0, [20, 20, 60, 70]); D(2, 0, [20, 20, 60, 70], 0.93); D(2, 0, [20, 20, 60, 69], 0.42)
    # 3: a difficult box that is the argmax (neither tp nor fp), beside a regular box with a lower IoU
    G(3, 0, [1, 1, 50, 50], 1); G(3, 0, [1, 6, 50, 55]); D(3, 0, [1, 1, 50, 51], 0.92)
    # 4: the first-ranked detection of the class sits on a difficult box: tp = fp = 0, the eps denominator
    G(4, 0, [100, 100, 150, 150], 1); D(4, 0, [100, 100, 150, 150], 0.999)
    # 5: three detections claim one box; the one in the middle of the arrival order has the highest score
    G(5, 0, [10, 10, 100, 100]); D(5, 0, [10, 10, 100, 98], 0.60); D(5, 0, [10, 10, 100, 97], 0.91); D(5, 0, [10, 10, 100, 99], 0.30)
    # 6: a detection in an image without boxes of its class
    G(6, 1, [1, 1, 30, 30]); D(6, 0, [5, 5, 40, 40], 0.50)
    # 7: equal IoU (0.8) to two different boxes: the earlier wins; the second detection is the later box itself and takes it
    G(7, 0, [1, 1, 10, 8]); G(7, 0, [1, 3, 10, 10]); D(7, 0, [1, 1, 10, 10], 0.90); D(7, 0, [1, 3, 10, 10], 0.20)
    # 8: the rounding of the result file decides: y2 + 1 = 5.04 is written as 5.0, IoU exactly 0.5 and no match (0.504 unrounded)
    G(8, 0, [1, 1, 10, 10]); dts.append((8, 0, [0., 0., 9., 4.04, 0.35]))
    # class 1: float32 coordinates whose + 1 lands on a decimal half, exactly (x.25, x.75: halves to even) and only in float32
    # (0.35f + 1 = 1.35f > 1.35 rounds up; in float64 the sum stays below 1.35); scores at exact binary x.xxx5 halves and near ones
    G(7, 1, [10, 10, 60, 60])
    for n, (c, s) in enumerate(((9.25, 0.0625), (9.75, 0.1875), (8.35, 0.3125), (8.45, 0.4375), (10.05, 0.5625), (9.15, 0.6875),
                                (8.65, 0.8125), (9.85, 0.9375), (0.35, 0.1235), (0.45, 0.2345), (0.55, 0.3455), (0.65, 0.4565))):
        dts.append((6 + n % 2, 1, [c, c + 0.5, c + 50.25, c + 49.75, s]))
    # class 2: boxes, no detections.  class 3: detections, every box difficult.  class 4: nothing.  class 5: detections, no box.
    G(0, 2, [1, 1, 20, 20]); G(3, 2, [5, 5, 80, 90], 1)
    G(1, 3, [1, 1, 40, 40], 1); G(2, 3, [10, 10, 90, 90], 1)
    D(1, 3, [1, 1, 40, 41], 0.80); D(2, 3, [200, 200, 240, 240], 0.70); D(5, 3, [1, 1, 10, 10], 0.60)
    D(0, 5, [1, 1, 10, 10], 0.55); D(4, 5, [3, 3, 30, 30], 0.45)
    return pack_gt(gts), pack_dt(dts, 9), 6, 9


def make_sets():
    few = lambda i, rng: int(rng.randint(3, 9))
    like = lambda i, rng: 200 if i % 40 == 7 else int(rng.randint(4, 40))
    return {'small': seeded_set(31, 40, 3, 3.0, few), 'edges': edges_set(), 'voc_like': seeded_set(32, 200, 20, 2.5, like)}


_CACHE = {}


def load_golden():
    """{set: (gt, dt, K, I, golden)} from the committed file; golden = rows (ND,5), cls_off (K+1), rec and prec (T,ND) in every
    class's sorted order, ap07 and ap_area (T,K) -- each written by the reference's voc_eval"""
    if not _CACHE:
        z = np.load(GOLDEN)
        for s in SETS:
            gt = {k: z['%s_in_gt_%s' % (s, k)] for k in GT_KEYS}
            dt = {k: z['%s_in_dt_%s' % (s, k)] for k in DT_KEYS}
            K, I = (int(v) for v in z['%s_shape' % s])
            _CACHE[s] = (gt, dt, K, I, {k: z['%s_%s' % (s, k)] for k in GOLDEN_KEYS})
    return _CACHE


def all_boxes_of(dt, K, I):
    """a set's detections as all_boxes[class][image] = (n,5) float32 rows (class 0 = background)"""
    out = [[np.zeros((0, 5), np.float32) for _ in range(I)] for _ in range(K + 1)]
    key = dt['category'].astype(np.int64) * I + dt['image']
    for kk in np.unique(key):
        out[int(kk // I) + 1][int(kk % I)] = dt['raw'][key == kk]
    return out


# ---- further seeded sets ----------------------------------------------------------------------------
SIZES_D = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024)
SIZES_G = (0, 1, 63, 64, 65, 255, 256)


def size_grid_set(seed, pairs):
    """one image per (D, G) pair, one class: exactly D detections and G boxes in that problem (a (0, 0) pair is no problem).  The
    boxes lie on a coarse grid so that several detections claim one box and equal IoUs occur; an eighth of them are difficult; the
    scores are quantised to 1/64 (ties within a problem)."""
    rng = np.random.RandomState(seed)
    gts, dts = [], []
    for i, (D, G) in enumerate(pairs):
        boxes = []
        for g in range(G):
            x, y = 1 + 40 * rng.randint(0, 6), 1 + 40 * rng.randint(0, 6)
            b = [x, y, x + rng.randint(20, 60), y + rng.randint(20, 60)]
            boxes.append(b)
            gts.append((i, 0, b, int(rng.rand() < 0.125)))
        for d in range(D):
            if boxes and rng.rand() < 0.8:
                b = boxes[rng.randint(len(boxes))]
                j = rng.randint(-6, 7, 4) * (rng.rand() < 0.7)
                row = [b[0] - 1 + j[0], b[1] - 1 + j[1], b[2] - 1 + abs(j[2]), b[3] - 1 + abs(j[3])]
            else:
                x, y = rng.uniform(0, 250, 2)
                row = [x, y, x + rng.uniform(10, 60), y + rng.uniform(10, 60)]
            dts.append((i, 0, row + [rng.randint(1, 65) / 64.0]))
    gt = pack_gt(gts) if gts else pack_gt([])
    dt = pack_dt(dts, len(pairs)) if dts else {'image': np.zeros(0, np.int32), 'category': np.zeros(0, np.int32), 'raw': np.zeros((0, 5), np.float32)}
    return gt, dt, 1, len(pairs)


def seam_counts(tile, chunk):
    """detections per class on both sides of every seam of the ordering (tile) and scan (chunk) launches"""
    return [1, tile - 1, tile, tile + 1, 2 * tile + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]


def class_count_set(seed, counts, per_problem=97):
    """class k gets counts[k] detections in all, at most per_problem per (image, class) problem, one or two boxes per problem (one
    in eight difficult), scores quantised to 1/50 (ties across every seam)"""
    rng = np.random.RandomState(seed)
    gts, dts = [], []
    n_img = max(1, max((c + per_problem - 1) // per_problem for c in counts))
    for k, c in enumerate(counts):
        left = c
        for i in range(n_img):
            if c == 0:
                break
            boxes = []
            for _ in range(1 + (i + k) % 2):
                w, h = np.exp(rng.uniform(np.log(8), np.log(300), 2))
                x, y = rng.uniform(1, 500, 2)
                b = [int(x), int(y), int(x + w), int(y + h)]
                boxes.append(b)
                gts.append((i, k, b, int(rng.rand() < 0.125)))
            n = min(left, per_problem)
            left -= n
            for _ in range(n):
                b = boxes[rng.randint(len(boxes))]
                s = 0.25
                w, h = b[2] - b[0] + 1, b[3] - b[1] + 1
                x, y = b[0] - 1 + rng.uniform(-s, s) * w, b[1] - 1 + rng.uniform(-s, s) * h
                w, h = w * np.exp(rng.uniform(-s, s)), h * np.exp(rng.uniform(-s, s))
                dts.append((i, k, [x, y, x + w - 1, y + h - 1, rng.randint(1, 51) / 50.0]))
        assert left == 0
    return pack_gt(gts), pack_dt(dts, n_img), len(counts), n_img


def tie_set():
    """equal rounded scores within an image and across images (scores quantised to 1/8), pairs that are equal only after the
    rounding (0.1231 and 0.1234) included"""
    gt, dt, K, I = seeded_set(41, 12, 2, 3.0, lambda i, rng: int(rng.randint(6, 14)), distinct=False, ties=8)
    sel = np.flatnonzero(dt['category'] == 0)
    dt['raw'][sel[::4], 4] = np.float32(0.1231)
    dt['raw'][sel[1::4], 4] = np.float32(0.1234)
    return gt, dt, K, I


def with_rows(dt, rows=None):
    """the restatement's detection dict: a set's dt plus its result rows"""
    return dict(dt, rows=result_rows(dt['raw']) if rows is None else rows)


# ---- the device, at the C ABI, with every operand in a guarded buffer ---------------------------------
def workspace_bytes(ND, T):
    return (8 * T * max(ND, 1) + 255) // 256 * 256


DEVICE_KEYS = ('dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det', 'order', 'rec', 'prec', 'npos', 'ap07', 'ap_area')
EXACT_KEYS = tuple(k for k in DEVICE_KEYS if k != 'ap_area')


def device_run(gt, rows, K, thresholds, ev):
    """sn_voc_match + sn_voc_accumulate on the CSR layout `ev` (the restatement's offsets and box permutation; `rows` are already
    class-major, image, row) -> the arrays named in DEVICE_KEYS; every operand guarded, the guards checked"""
    import torch
    from sniper_amd import hip
    gp = ev['gt_perm']
    thrs = np.asarray(thresholds, np.float64)
    T, ND, NG, P = len(thrs), len(rows), len(gp), len(ev['prob_cat'])
    assert P >= 1
    dcount, gcount = np.diff(ev['dt_off']), np.diff(ev['gt_off'])
    per_class = np.diff(ev['dt_off'][ev['cat_off']].astype(np.int64))
    G = Guarded()
    d_box, d_score = G.put(np.ascontiguousarray(rows[:, :4], np.float64)), G.put(np.ascontiguousarray(rows[:, 4], np.float64))
    d_gt, d_diff = G.put(gt['bbox'][gp].astype(np.float64).reshape(-1, 4)), G.put((gt['difficult'][gp] != 0).astype(np.uint8))
    d_dt_off, d_gt_off, d_cat_off = (G.put(ev[k].astype(np.int32)) for k in ('dt_off', 'gt_off', 'cat_off'))
    d_thr = G.put(thrs)
    shapes = {'dt_best': ((ND,), np.int32), 'dt_iou': ((ND,), np.float64), 'dt_tp': ((T, ND), np.uint8), 'dt_fp': ((T, ND), np.uint8),
              'gt_det': ((T, NG), np.int32), 'order': ((ND,), np.int32), 'rec': ((T, ND), np.float64), 'prec': ((T, ND), np.float64),
              'npos': ((K,), np.int32), 'ap07': ((T, K), np.float64), 'ap_area': ((T, K), np.float64)}
    o = {k: G.out(*shapes[k]) for k in DEVICE_KEYS}
    need = int(hip.query('sn_voc_accumulate_workspace_bytes', ND, T))
    assert need == workspace_bytes(ND, T)
    ws = G.out((need,), np.uint8)
    hip.call('sn_voc_match', d_box, d_score, d_dt_off, d_gt, d_diff, d_gt_off, d_thr, P, T, int(dcount.max()), int(gcount.max()), ND, NG,
             o['dt_best'], o['dt_iou'], o['dt_tp'], o['dt_fp'], o['gt_det'], hip.stream())
    hip.call('sn_voc_accumulate', d_score, d_dt_off, d_gt_off, d_cat_off, d_diff, o['dt_tp'], o['dt_fp'], np.arange(0., 1.1, 0.1), P, K, T,
             int(per_class.max()), ND, NG, ws, need, o['order'], o['rec'], o['prec'], o['npos'], o['ap07'], o['ap_area'], hip.stream())
    torch.cuda.synchronize()
    G.check()
    return {k: Guarded.read(o[k], *shapes[k]) for k in DEVICE_KEYS}


def same_bits(a, b):
    """equal on the bits, except that a nan equals any nan (sign and payload are not compared)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == 'f':
        na, nb = np.isnan(a), np.isnan(b)
        return bool(np.array_equal(na, nb) and np.where(na, 0, a).tobytes() == np.where(nb, 0, b).tobytes())
    return a.tobytes() == b.tobytes()


def assert_same_bits(got, want, keys, what=''):
    for k in keys:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if not same_bits(a, b):
            bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == 'f' else (a == b)))
            raise AssertionError('%s %s: %d of %d entries differ, first at %s: got %r want %r' % (
                what, k, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))


def recall_changes(rec, cls_off):
    """(T,K): the number n of recall changes of every curve, sentinels included (voc_ap's `i`): the terms of the area sum"""
    T, K = rec.shape[0], len(cls_off) - 1
    n = np.zeros((T, K), np.int64)
    for t in range(T):
        for k in range(K):
            mrec = np.concatenate(([0.], rec[t, cls_off[k]:cls_off[k + 1]], [1.]))
            n[t, k] = np.count_nonzero(mrec[1:] != mrec[:-1])
    return n


def assert_area_within_bound(got, want, n, what=''):
    """|ap_area - reference| <= 2 * (n - 1) * 2^-53: every term is >= 0 and every partial sum <= 1, so any summation order errs by at
    most (n - 1) * 2^-53, and numpy's pairwise order and the device's may differ by twice that; nan where the reference has nan"""
    assert got.shape == want.shape == n.shape, (what, got.shape, want.shape, n.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, 'nan positions', got, want)
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = 2.0 * np.maximum(n[ok] - 1, 0) * 2.0 ** -53
    assert (err <= bound).all(), (what, 'ap_area', err.max(), bound[np.argmax(err - bound)])
