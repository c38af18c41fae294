"""What the COCO mask evaluation tests and tests/golden/make_cocosegm_golden.py share: the hand-made, edge and seeded sets, the
loader of tests/golden/cocosegm_v1.npz, and the device run at the C ABI with every operand between guard bytes.

A SET is a dict: K, I, sizes (I,2) int32 = h, w of every image; gt = list of annotations in annotation-id order, each a dict(image,
category, area, iscrowd, ignore, seg) with seg = ('mask', (h,w) uint8 bitmap) | ('string', bitmap: handed to the evaluator as
compressed string counts) | ('poly', [flat x0, y0, x1, y1, ... lists]); dt = list of dict(image, category, score, mask bitmap).
Bitmaps become counts through the REFERENCE's rleEncode in the golden maker; the tests read the counts from the golden."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cocosegm_v1.npz')
SETS = ('hand', 'edge', 'seeded')
FORM_COUNTS, FORM_STRING, FORM_POLY = 0, 1, 2
RESULT_KEYS = ('dt_rank', 'dt_scores', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore', 'precision', 'recall', 'stats')
QUIRK_GT, QUIRK_DT = (35, 8, 57), (40, 2, 58)          # h = w = 10: two common pixels, and the reference says 0


def _bitmap(h, w, *rects):
    """ones in the rectangles (y0, x0, y1, x1), both ends inclusive"""
    m = np.zeros((h, w), np.uint8)
    for y0, x0, y1, x1 in rects:
        m[y0:y1 + 1, x0:x1 + 1] = 1
    return m


def from_counts(counts, h, w):
    """counts -> (h,w) bitmap (column-major runs, zeros first)"""
    flat = np.repeat(np.arange(len(counts)) % 2, np.asarray(counts, np.int64)).astype(np.uint8)
    assert flat.size == h * w
    return np.ascontiguousarray(flat.reshape(w, h).T)


def hand_set():
    """Seven images small enough to draw on paper, three categories."""
    sizes = [(6, 6), (10, 10), (8, 8), (8, 8), (6, 6), (6, 6), (6, 8)]
    gt, dt = [], []
    G = lambda i, k, m, area=None, crowd=0, ign=0, form='mask': gt.append(dict(
        image=i, category=k, area=float(m.sum() if area is None else area), iscrowd=crowd, ignore=ign, seg=(form, m)))
    D = lambda i, k, m, s: dt.append(dict(image=i, category=k, score=float(s), mask=m))
    B = lambda i, *r: _bitmap(sizes[i][0], sizes[i][1], *r)
    # 0: an identical mask (IoU 1: matched at every threshold) and a disjoint one (unmatched at every threshold)
    G(0, 0, B(0, (1, 1, 3, 3))); D(0, 0, B(0, (1, 1, 3, 3)), 0.9); D(0, 0, B(0, (5, 5, 5, 5)), 0.8)
    # 1: the column-wrap pair: the masks share pixels 40 and 41, their rleToBbox boxes do not overlap, the IoU is 0
    G(1, 0, from_counts(QUIRK_GT, 10, 10)); D(1, 0, from_counts(QUIRK_DT, 10, 10), 0.7)
    # 2: IoU exactly 0.75 and exactly 0.5 against a 4 x 4 square; the second box is matched by nothing
    G(2, 1, B(2, (0, 0, 3, 3))); G(2, 1, B(2, (6, 6, 7, 7)))
    D(2, 1, B(2, (0, 0, 3, 2)), 0.9); D(2, 1, B(2, (0, 0, 3, 1)), 0.5)
    # 3: a crowd region matched by two detections (intersection / detection area = 1) beside a regular object
    G(3, 1, B(3, (0, 0, 7, 4)), crowd=1); G(3, 1, B(3, (2, 6, 5, 7)))
    D(3, 1, B(3, (1, 1, 2, 2)), 0.9); D(3, 1, B(3, (4, 2, 6, 4)), 0.8); D(3, 1, B(3, (2, 6, 5, 7)), 0.7); D(3, 1, B(3, (0, 4, 1, 6)), 0.6)
    # 4, 5: ground truth without detections, and the reverse
    G(4, 2, B(4, (0, 0, 2, 2))); D(5, 2, B(5, (3, 3, 5, 5)), 0.9)
    # 6: an object of two parts; a detection that covers one part (IoU 4 / 8), one that covers both
    G(6, 2, B(6, (0, 0, 1, 1), (4, 5, 5, 6))); D(6, 2, B(6, (0, 0, 1, 1)), 0.4); D(6, 2, B(6, (0, 0, 1, 1), (4, 5, 5, 6)), 0.3)
    # an identical pair with an ignore flag, equal scores
    G(6, 0, B(6, (2, 2, 4, 4)), ign=1); D(6, 0, B(6, (2, 2, 4, 4)), 0.5); D(6, 0, B(6, (2, 2, 4, 3)), 0.5)
    return dict(K=3, I=len(sizes), sizes=np.array(sizes, np.int32), gt=gt, dt=dt)


EDGE_CASES = ('polygon wholly outside', 'polygon partly outside on every side', 'negative coordinates in the truncation band',
              'half-integer vertices', 'repeated vertex', 'explicit closing vertex', 'polygon of 1 point', 'polygon of 2 points',
              'zero area', 'two overlapping parts', 'a part inside another', 'polygon covering the last pixel', 'full image height',
              'h = 1 image', 'w = 1 image', 'all-zero detection', 'all-one detection', 'crowd as uncompressed counts',
              'crowd as string counts')


def edge_set():
    """One case per annotation; `case` names it (make_cocosegm_golden.py asserts that every name of EDGE_CASES is present)."""
    sizes = [(12, 16), (1, 9), (9, 1), (10, 10)]
    gt, dt = [], []

    def P(i, k, polys, case, area=20.0):
        gt.append(dict(image=i, category=k, area=float(area), iscrowd=0, ignore=0, seg=('poly', [[float(v) for v in p] for p in polys]),
                       case=case))

    def G(i, k, m, case, crowd=0, form='mask'):
        gt.append(dict(image=i, category=k, area=float(m.sum()), iscrowd=crowd, ignore=0, seg=(form, m), case=case))
    D = lambda i, k, m, s, case=None: dt.append(dict(image=i, category=k, score=float(s), mask=m, case=case))
    B = lambda i, *r: _bitmap(sizes[i][0], sizes[i][1], *r)
    P(0, 0, [[20, 20, 30, 20, 30, 30, 20, 30]], 'polygon wholly outside')
    P(0, 0, [[-3, -2, 19, -4, 18, 15, -5, 14]], 'polygon partly outside on every side')
    P(0, 0, [[-0.25, -0.15, 6.2, -0.11, 6.1, 5.3, -0.29, 5.2]], 'negative coordinates in the truncation band')
    P(0, 0, [[2.5, 3.5, 9.5, 3.5, 9.5, 8.5, 2.5, 8.5]], 'half-integer vertices')
    P(0, 1, [[1, 1, 8, 1, 8, 1, 8, 7, 1, 7]], 'repeated vertex')
    P(0, 1, [[3, 2, 12, 2, 12, 9, 3, 9, 3, 2]], 'explicit closing vertex')
    P(0, 1, [[5, 5]], 'polygon of 1 point')
    P(0, 1, [[2, 2, 11, 9]], 'polygon of 2 points')
    P(0, 1, [[1, 1, 9, 9, 5, 5]], 'zero area')
    P(0, 2, [[1, 1, 9, 1, 9, 7, 1, 7], [5, 4, 14, 4, 14, 10, 5, 10]], 'two overlapping parts')
    P(0, 2, [[1, 1, 14, 1, 14, 10, 1, 10], [4, 3, 8, 3, 8, 7, 4, 7]], 'a part inside another')
    P(0, 2, [[10, 6, 16, 6, 16, 12, 10, 12]], 'polygon covering the last pixel')
    P(0, 2, [[4, 0, 9, 0, 9, 12, 4, 12]], 'full image height')
    G(1, 0, B(1, (0, 2, 0, 5)), 'h = 1 image'); D(1, 0, B(1, (0, 3, 0, 6)), 0.8); D(1, 0, B(1, (0, 8, 0, 8)), 0.3)
    G(2, 0, B(2, (1, 0, 6, 0)), 'w = 1 image'); D(2, 0, B(2, (1, 0, 6, 0)), 0.9); D(2, 0, B(2, (0, 0, 0, 0)), 0.2)
    G(3, 1, B(3, (0, 0, 9, 5)), 'crowd as uncompressed counts', crowd=1)
    G(3, 2, B(3, (2, 1, 8, 8)), 'crowd as string counts', crowd=1, form='string')
    G(3, 1, B(3, (3, 7, 6, 9)), None); G(3, 2, B(3, (0, 9, 9, 9)), None)
    D(3, 1, B(3), 0.9, 'all-zero detection'); D(3, 1, B(3, (0, 0, 9, 9)), 0.8, 'all-one detection')
    D(3, 1, B(3, (1, 1, 4, 4)), 0.7); D(3, 1, B(3, (3, 7, 6, 9)), 0.6)
    D(3, 2, B(3, (3, 2, 5, 5)), 0.9); D(3, 2, B(3, (0, 9, 9, 9)), 0.5); D(3, 2, B(3, (0, 0, 1, 1)), 0.4)
    # detections on the polygons of image 0: a copy of what the polygon covers is made by the golden maker (mask = None -> the
    # reference's own RLE of the annotation named by `of`, which makes a pair of IoU 1), plus plain rectangles
    for n, a in enumerate(gt):
        if a['image'] == 0 and n % 2 == 0:
            dt.append(dict(image=0, category=a['category'], score=0.9 - 0.01 * n, mask=None, of=n, case=None))
    D(0, 0, B(0, (0, 0, 5, 6)), 0.55); D(0, 1, B(0, (2, 3, 9, 12)), 0.45); D(0, 2, B(0, (0, 4, 11, 9)), 0.35); D(0, 2, B(0, (11, 0, 11, 0)), 0.2)
    return dict(K=3, I=len(sizes), sizes=np.array(sizes, np.int32), gt=gt, dt=dt)


def _blob(rng, h, w):
    """an ellipse or a rectangle of random size, sometimes with a second part"""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(1 + (rng.rand() < 0.25)):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(2, h / 2.5), rng.uniform(2, w / 2.5)
        if rng.rand() < 0.5:
            m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        else:
            m |= (np.abs(yy - cy) <= ry) & (np.abs(xx - cx) <= rx)
    if not m.any():
        m[int(min(cy, h - 1)), int(min(cx, w - 1))] = True
    return m.astype(np.uint8)


def _perturb(rng, m):
    """a shifted copy with a random rectangle added or removed"""
    h, w = m.shape
    s = (0, 1, 3)[rng.randint(3)]
    out = np.zeros_like(m)
    dy, dx = rng.randint(-s, s + 1, 2)
    src = m[max(0, -dy):h - max(0, dy), max(0, -dx):w - max(0, dx)]
    out[max(0, dy):max(0, dy) + src.shape[0], max(0, dx):max(0, dx) + src.shape[1]] = src
    if rng.rand() < 0.6:
        y0, x0 = rng.randint(h), rng.randint(w)
        y1, x1 = min(h, y0 + rng.randint(1, 6)), min(w, x0 + rng.randint(1, 6))
        out[y0:y1, x0:x1] = rng.rand() < 0.5
    return out


def seeded_set(seed=21, n_img=24, n_cat=4):
    """Images of at most 64 x 48 pixels.  The annotation's own area is its pixel count times 1, 3, 10 or 40, so that all three
    area ranges hold objects; 10 % crowd, 4 % with the ignore flag; a perturbed copy for 85 % of the objects, a third as many false
    positives; scores quantised to 1/50 so that ties occur."""
    rng = np.random.RandomState(seed)
    sizes, gt, dt = [], [], []
    for i in range(n_img):
        h, w = int(rng.randint(20, 49)), int(rng.randint(24, 65))
        sizes.append((h, w))
        for _ in range(max(1, rng.poisson(4.5))):
            k = int(rng.randint(n_cat))
            m = _blob(rng, h, w)
            area = float(m.sum()) * (1, 3, 10, 40)[rng.randint(4)]
            gt.append(dict(image=i, category=k, area=area, iscrowd=int(rng.rand() < 0.10), ignore=int(rng.rand() < 0.04),
                           seg=('string' if rng.rand() < 0.2 else 'mask', m)))
            if rng.rand() < 0.85:
                dt.append(dict(image=i, category=k, score=round(float(rng.randint(1, 51)) / 50, 8), mask=_perturb(rng, m)))
            if rng.rand() < 0.30:
                dt.append(dict(image=i, category=int(rng.randint(n_cat)), score=round(float(rng.randint(1, 51)) / 50, 8),
                               mask=_blob(rng, h, w)))
    return dict(K=n_cat, I=n_img, sizes=np.array(sizes, np.int32), gt=gt, dt=dt)


def make_sets():
    return {'hand': hand_set(), 'edge': edge_set(), 'seeded': seeded_set()}


# ---- the golden ---------------------------------------------------------------------------------------
_CACHE = {}


def _split(pool, off):
    return [pool[off[n]:off[n + 1]] for n in range(len(off) - 1)]


def load_golden():
    """{set: dict} from the committed file: K, I, sizes; gt_* arrays (image, category, area, iscrowd, ignore, form) and gt_counts (the
    reference's counts of every annotation), gt_strings (bytes, '' where the form is not a string), gt_polys (list of float64 vertex
    arrays per annotation, [] where the form is not polygons); dt_* arrays (image, category, score, area, bbox (ND,4)) and dt_counts;
    iou, iou_off (P+1): the reference's rleIou of every problem, detection-major in arrival order; the RESULT_KEYS arrays."""
    if not _CACHE:
        z = np.load(GOLDEN)
        for s in SETS:
            g = lambda k: z['%s_%s' % (s, k)]
            K, I = (int(v) for v in g('shape'))
            d = dict(K=K, I=I, sizes=g('sizes'))
            for k in ('gt_image', 'gt_category', 'gt_area', 'gt_iscrowd', 'gt_ignore', 'gt_form', 'dt_image', 'dt_category', 'dt_score',
                      'dt_area', 'dt_bbox', 'iou', 'iou_off'):
                d[k] = g(k)
            d['gt_counts'] = _split(g('gt_cnts'), g('gt_cnt_off'))
            d['dt_counts'] = _split(g('dt_cnts'), g('dt_cnt_off'))
            d['gt_strings'] = [bytes(b).decode('ascii') for b in _split(g('gt_str'), g('gt_str_off'))]
            polys = _split(g('poly_xy'), g('poly_off'))
            d['gt_polys'] = [polys[a:b] for a, b in zip(g('ann_poly_off')[:-1], g('ann_poly_off')[1:])]
            res = {k: g('res_' + k) for k in RESULT_KEYS}
            res['precision'] = np.ascontiguousarray(res['precision'].transpose(0, 4, 1, 2, 3))     # stored (T,K,A,M,R)
            d['res'] = res
            _CACHE[s] = d
    return _CACHE


def segmentations(d, polygons=True):
    """the annotations' `segmentation` entries as the evaluator takes them: uncompressed counts, string counts, or polygon lists
    (polygons=False: the reference's counts of the polygon instead)"""
    out = []
    for n in range(len(d['gt_image'])):
        size = [int(v) for v in d['sizes'][d['gt_image'][n]]]
        form = int(d['gt_form'][n])
        if form == FORM_STRING:
            out.append({'size': size, 'counts': d['gt_strings'][n]})
        elif form == FORM_POLY and polygons:
            out.append([[float(v) for v in p] for p in d['gt_polys'][n]])
        else:
            out.append({'size': size, 'counts': [int(c) for c in d['gt_counts'][n]]})
    return out


def gt_dict(d, polygons=True):
    return {'image': d['gt_image'], 'category': d['gt_category'], 'area': d['gt_area'], 'iscrowd': d['gt_iscrowd'],
            'ignore': d['gt_ignore'], 'segmentation': segmentations(d, polygons)}


def detections_of(d):
    """-> all_boxes[class][image] (n,5) rows (the box columns are not read by the mask evaluation: zeros) and all_masks[class][image]
    = lists of RLE dicts, class 0 = background"""
    K, I = d['K'], d['I']
    boxes = [[np.zeros((0, 5)) for _ in range(I)] for _ in range(K + 1)]
    masks = [[[] for _ in range(I)] for _ in range(K + 1)]
    for n in range(len(d['dt_image'])):
        k, i = int(d['dt_category'][n]) + 1, int(d['dt_image'][n])
        boxes[k][i] = np.concatenate((boxes[k][i], [[0, 0, 0, 0, float(d['dt_score'][n])]]))
        masks[k][i].append({'size': [int(v) for v in d['sizes'][i]], 'counts': d['dt_counts'][n]})
    return boxes, masks


def ref_inputs(d):
    """the golden's set in the form tests/coco_segm_ref.py evaluates: (gt, dt) dicts with `rle` lists of uint32 counts and `hw`"""
    gt = {'image': d['gt_image'], 'category': d['gt_category'], 'area': d['gt_area'], 'iscrowd': d['gt_iscrowd'], 'ignore': d['gt_ignore'],
          'rle': d['gt_counts'], 'hw': d['sizes'][d['gt_image']].reshape(-1, 2)}
    dt = {'image': d['dt_image'], 'category': d['dt_category'], 'score': d['dt_score'], 'rle': d['dt_counts'],
          'hw': d['sizes'][d['dt_image']].reshape(-1, 2)}
    return gt, dt


# ---- the device, at the C ABI, with every operand in a guarded buffer ---------------------------------
def pool(rles):
    """list of count arrays -> (uint32 pool, (N+1) int32 offsets)"""
    off = np.zeros(len(rles) + 1, np.int64)
    np.cumsum([len(r) for r in rles], out=off[1:])
    cnts = np.concatenate([np.asarray(r, np.uint32) for r in rles]) if len(rles) and off[-1] else np.zeros(0, np.uint32)
    return cnts, off.astype(np.int32)


def device_stats(rles, hw, score=None):
    """sn_rle_stats -> rows6 (N,6), cum2 (total,2)"""
    import torch
    from coco_eval_util import Guarded
    from sniper_amd import hip
    cnts, off = pool(rles)
    N, total = len(rles), int(off[-1])
    hw = np.asarray(hw, np.int32).reshape(N, 2)
    G = Guarded()
    d_c, d_off, d_hw = G.put(cnts), G.put(off), G.put(hw)
    d_s = G.put(np.asarray(score, np.float64)) if score is not None else None
    o_rows, o_cum = G.out((N, 6), np.float64), G.out((total, 2), np.uint32)
    hip.call('sn_rle_stats', d_c, d_off, d_hw, d_s, N, total, int((hw[:, 0].astype(np.int64) * hw[:, 1]).max()), o_rows, o_cum, hip.stream())
    torch.cuda.synchronize()
    G.check()
    return Guarded.read(o_rows, (N, 6), np.float64), Guarded.read(o_cum, (total, 2), np.uint32)


def device_iou(ev, gt, dt):
    """sn_rle_stats on both sides + sn_rle_iou over the problems of `ev` (the restatement's CSR layout) -> (iou pool, iou_off,
    dt rows6, gt rows6) with the masks in CSR order"""
    import torch
    from coco_eval_util import Guarded
    from sniper_amd import hip
    dp, gp = ev['dt_perm'], ev['gt_perm']
    d_rles, g_rles = [dt['rle'][n] for n in dp], [gt['rle'][n] for n in gp]
    d_rows, d_cum = device_stats(d_rles, dt['hw'][dp], np.asarray(dt['score'], np.float64)[dp]) if len(dp) else (np.zeros((0, 6)), np.zeros((0, 2), np.uint32))
    g_rows, g_cum = device_stats(g_rles, gt['hw'][gp]) if len(gp) else (np.zeros((0, 6)), np.zeros((0, 2), np.uint32))
    flags = ((np.asarray(gt['iscrowd'])[gp] != 0).astype(np.uint8) | ((np.asarray(gt['ignore'])[gp] != 0).astype(np.uint8) << 1))
    iou_off = np.concatenate([[0], np.cumsum(np.diff(ev['dt_off']).astype(np.int64) * np.diff(ev['gt_off']))])
    n_pairs, P = int(iou_off[-1]), len(ev['dt_off']) - 1
    G = Guarded()
    args = [G.put(d_cum), G.put(pool(d_rles)[1]), G.put(d_rows), G.put(g_cum), G.put(pool(g_rles)[1]), G.put(g_rows), G.put(flags),
            G.put(ev['dt_off'].astype(np.int32)), G.put(ev['gt_off'].astype(np.int32)), G.put(iou_off.astype(np.int32))]
    o_iou = G.out((n_pairs,), np.float64)
    hip.call('sn_rle_iou', *(args + [P, n_pairs, o_iou, hip.stream()]))
    torch.cuda.synchronize()
    G.check()
    return Guarded.read(o_iou, (n_pairs,), np.float64), iou_off.astype(np.int32), d_rows, g_rows


def device_match(ev, gt, dt_rows6, iou, iou_off, K, params):
    """sn_coco_match_iou + sn_coco_accumulate on the CSR layout `ev` -> the arrays of coco_eval_util.DEVICE_KEYS"""
    import torch
    from coco_eval_util import Guarded, workspace_bytes
    from sniper_amd import hip
    gp = ev['gt_perm']
    area = np.asarray(gt['area'], np.float64)[gp]
    flags = ((np.asarray(gt['iscrowd'])[gp] != 0).astype(np.uint8) | ((np.asarray(gt['ignore'])[gp] != 0).astype(np.uint8) << 1))
    thr, rec = np.asarray(params.iouThrs, np.float64), np.asarray(params.recThrs, np.float64)
    rng = np.asarray(params.areaRng, np.float64).reshape(-1, 2)
    max_dets = np.asarray(params.maxDets, np.int32)
    T, R, A, M = len(thr), len(rec), len(rng), len(max_dets)
    P, NK, NG = len(ev['prob_cat']), int(ev['kp_off'][-1]), len(gp)
    dcount, gcount = np.diff(ev['dt_off']), np.diff(ev['gt_off'])
    kept_per_cat = np.diff(ev['kp_off'][ev['cat_off']].astype(np.int64))
    G = Guarded()
    d_dt, d_area, d_flags = G.put(np.asarray(dt_rows6, np.float64).reshape(-1, 6)), G.put(area), G.put(flags)
    d_dt_off, d_gt_off, d_kp_off, d_cat_off = (G.put(ev[k].astype(np.int32)) for k in ('dt_off', 'gt_off', 'kp_off', 'cat_off'))
    d_iou, d_iou_off = G.put(np.asarray(iou, np.float64)), G.put(np.asarray(iou_off, np.int32))
    d_thr, d_rec, d_rng = G.put(thr), G.put(rec), G.put(rng)
    o_rank, o_dtm, o_dtig = G.out((NK,), np.int32), G.out((A, T, NK), np.int32), G.out((A, T, NK), np.uint8)
    o_gtm, o_gtig = G.out((A, T, NG), np.int32), G.out((A, NG), np.uint8)
    o_pr, o_rc = G.out((T, R, K, A, M), np.float64), G.out((T, K, A, M), np.float64)
    need = workspace_bytes(NK, T, A)
    ws = G.out((need,), np.uint8)
    hip.call('sn_coco_match_iou', d_dt, d_dt_off, d_kp_off, d_area, d_flags, d_gt_off, d_iou, d_iou_off, d_thr, d_rng, P, T, A,
             int(max_dets[-1]), int(dcount.max()), int(gcount.max()), NK, NG, o_rank, o_dtm, o_dtig, o_gtm, o_gtig, hip.stream())
    hip.call('sn_coco_accumulate', d_dt, d_dt_off, d_kp_off, d_gt_off, d_cat_off, o_rank, o_dtm, o_dtig, o_gtig, d_rec, max_dets, P, K,
             T, A, M, R, int(max_dets[-1]), int(kept_per_cat.max()), NK, NG, ws, need, o_pr, o_rc, hip.stream())
    torch.cuda.synchronize()
    G.check()
    rd = Guarded.read
    return {'dt_rank': rd(o_rank, (NK,), np.int32), 'dt_match': rd(o_dtm, (A, T, NK), np.int32), 'dt_ignore': rd(o_dtig, (A, T, NK), np.uint8),
            'gt_match': rd(o_gtm, (A, T, NG), np.int32), 'gt_ignore': rd(o_gtig, (A, NG), np.uint8),
            'precision': rd(o_pr, (T, R, K, A, M), np.float64), 'recall': rd(o_rc, (T, K, A, M), np.float64)}


def roidb_of(d, with_areas=True):
    """the golden's set as a roidb with run-length encoded `gt_masks` (a roidb has no ignore flag: the caller compares with an
    evaluation whose flags are zero) -> (roidb, num_classes)"""
    segs = segmentations(d, polygons=False)
    roidb = []
    for i in range(d['I']):
        rows = np.flatnonzero(d['gt_image'] == i)
        r = {'height': int(d['sizes'][i][0]), 'width': int(d['sizes'][i][1]), 'boxes': np.zeros((len(rows), 4)),
             'gt_classes': d['gt_category'][rows].astype(np.int32) + 1, 'gt_iscrowd': d['gt_iscrowd'][rows], 'gt_masks': [segs[n] for n in rows]}
        if with_areas:
            r['gt_areas'] = d['gt_area'][rows]
        roidb.append(r)
    return roidb, d['K'] + 1
