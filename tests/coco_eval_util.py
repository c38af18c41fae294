"""What the COCO evaluation tests and tests/golden/make_cocoeval_golden.py share: the seeded generator of ground truth and
detections, the hand-made problems, and the loader of tests/golden/cocoeval_v1.npz.

A SET is (gt, dt, K, I): gt = dict(image, category, bbox (n,4) xywh, area, iscrowd, ignore), dt = dict(image, category, bbox, score,
area), both in annotation-id order, images and categories as 0-based indices."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cocoeval_v1.npz')
GT_KEYS = ('image', 'category', 'bbox', 'area', 'iscrowd', 'ignore')
DT_KEYS = ('image', 'category', 'bbox', 'score', 'area')
RESULT_KEYS = ('dt_rank', 'dt_scores', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore', 'precision', 'recall', 'stats')
SETS = ('small', 'large', 'hand')


def _pack(rows, keys, int_keys):
    out = {}
    for n, k in enumerate(keys):
        col = [r[n] for r in rows]
        if k == 'bbox':
            out[k] = np.array(col, np.float64).reshape(-1, 4)
        elif k in int_keys:
            out[k] = np.array(col, np.int32)
        else:
            out[k] = np.array(col, np.float64)
    return out


def pack_gt(rows):
    return _pack(rows, GT_KEYS, ('image', 'category', 'iscrowd', 'ignore'))


def pack_dt(rows):
    return _pack(rows, DT_KEYS, ('image', 'category'))


def seeded_set(seed, n_img, n_cat, gt_per_img, dets_per_problem=None):
    """Boxes of 8..300 pixels (all three area ranges); 10 % crowd, 5 % with the ignore flag; a detection for 85 % of the boxes,
    jittered by +-s*w, +-s*h in position and exp(U(-s, s)) in size with s from {0.03, 0.08, 0.2}; a quarter of the detections are
    random boxes; scores quantised to 1/50 so that ties occur.  dets_per_problem: (D, G) puts exactly D detections and G boxes into
    every (image, category) pair instead (the kernel's size grid)."""
    rng = np.random.RandomState(seed)
    gts, dts = [], []

    def box():
        w, h = np.exp(rng.uniform(np.log(8), np.log(300), 2))
        x, y = rng.uniform(0, 500, 2)
        return [round(float(v), 2) for v in (x, y, w, h)]

    def det_of(b):
        s = (0.03, 0.08, 0.2)[rng.randint(3)]
        x = b[0] + rng.uniform(-s, s) * b[2]
        y = b[1] + rng.uniform(-s, s) * b[3]
        w = b[2] * np.exp(rng.uniform(-s, s))
        h = b[3] * np.exp(rng.uniform(-s, s))
        return [round(float(v), 1) for v in (x, y, w, h)]

    def score():
        return round(float(rng.randint(1, 51)) / 50, 8)

    for i in range(n_img):
        if dets_per_problem is None:
            pairs = [(int(rng.randint(n_cat)), None) for _ in range(rng.poisson(gt_per_img))]
        else:
            pairs = [(k, dets_per_problem) for k in range(n_cat)]
        for k, dg in pairs:
            n_box = 1 if dg is None else dg[1]
            mine = []
            for _ in range(n_box):
                b = box()
                area = round(b[2] * b[3] * float(rng.uniform(0.4, 1.0)), 1)
                gts.append((i, k, b, area, int(rng.rand() < 0.10), int(rng.rand() < 0.05)))
                mine.append(b)
            if dg is None:
                if rng.rand() < 0.85:
                    b = det_of(mine[0])
                    dts.append((i, k, b, score(), b[2] * b[3]))
                if rng.rand() < 0.30:                       # about a quarter of all detections
                    b = [round(v, 1) for v in box()]
                    dts.append((i, int(rng.randint(n_cat)), b, score(), b[2] * b[3]))
            else:
                for n in range(dg[0]):
                    if mine and rng.rand() < 0.75:
                        b = det_of(mine[rng.randint(len(mine))])
                    else:
                        b = [round(v, 1) for v in box()]
                    dts.append((i, k, b, score(), b[2] * b[3]))
    return pack_gt(gts), pack_dt(dts), n_cat, n_img


def hand_set():
    """The hand-made problems: one case per image, six categories (category 4 wholly absent, every box of category 5 ignored)."""
    gts, dts = [], []
    G = lambda i, k, b, area=None, crowd=0, ign=0: gts.append((i, k, [float(v) for v in b], float(b[2] * b[3] if area is None else area), crowd, ign))
    D = lambda i, k, b, s, area=None: dts.append((i, k, [float(v) for v in b], float(s), float(b[2] * b[3] if area is None else area)))
    # 0, 1: IoU exactly 0.5 and exactly 0.75 (50/100, 75/100), with a second lower-scored detection that would also match
    G(0, 0, [0, 0, 10, 10]); D(0, 0, [0, 0, 10, 5], 0.9); D(0, 0, [0, 0, 10, 9], 0.5)
    G(1, 0, [0, 0, 10, 10]); D(1, 0, [0, 0, 10, 7.5], 0.9); D(1, 0, [0, 0, 10, 6], 0.5)
    # 2: identical boxes, IoU exactly 1 (the threshold is min(t, 1 - 1e-10))
    G(2, 0, [3, 4, 20, 30]); D(2, 0, [3, 4, 20, 30], 0.8)
    # 3: two boxes with IoU 0.8 each to one detection -- the later must win; a second detection then takes the earlier one
    G(3, 0, [0, 0, 10, 8]); G(3, 0, [0, 2, 10, 8]); D(3, 0, [0, 0, 10, 10], 0.9); D(3, 0, [0, 0, 10, 8], 0.7)
    # 4: areas exactly 32^2 and 96^2, matched and unmatched, boxes and detections
    G(4, 1, [0, 0, 32, 32]); G(4, 1, [100, 100, 96, 96]); G(4, 1, [300, 0, 40, 40], area=1024.0); G(4, 1, [300, 100, 50, 50], area=9216.0)
    D(4, 1, [0, 0, 32, 32], 0.9); D(4, 1, [100, 100, 96, 96], 0.8); D(4, 1, [500, 500, 32, 32], 0.7); D(4, 1, [700, 700, 96, 96], 0.6)
    D(4, 1, [300, 0, 40, 40], 0.5, area=1024.0); D(4, 1, [300, 100, 50, 50], 0.4, area=9216.0)
    # 5: 130 detections (more than maxDets[-1] = 100), tied scores, three boxes
    rng = np.random.RandomState(5)
    boxes = [[10, 10, 60, 40], [200, 50, 30, 90], [100, 200, 120, 110]]
    for b in boxes:
        G(5, 1, b)
    for n in range(130):
        b = boxes[n % 3]
        jit = [round(float(b[0] + rng.uniform(-0.3, 0.3) * b[2]), 1), round(float(b[1] + rng.uniform(-0.3, 0.3) * b[3]), 1),
               round(float(b[2] * np.exp(rng.uniform(-0.3, 0.3))), 1), round(float(b[3] * np.exp(rng.uniform(-0.3, 0.3))), 1)]
        D(5, 1, jit, round(float(rng.randint(1, 21)) / 20, 8))
    # 6, 7: ground truth without detections, and the reverse
    G(6, 2, [0, 0, 50, 50]); G(6, 2, [60, 60, 20, 20])
    D(7, 2, [0, 0, 50, 50], 0.9); D(7, 2, [10, 10, 200, 200], 0.3)
    G(8, 2, [5, 5, 40, 40]); D(8, 2, [6, 6, 40, 40], 0.6)
    # 9: a crowd box matched by two detections (IoU with a crowd = intersection / detection area = 1), beside a regular box
    G(9, 3, [0, 0, 100, 100], crowd=1); G(9, 3, [200, 200, 30, 30])
    D(9, 3, [10, 10, 20, 20], 0.9); D(9, 3, [50, 50, 20, 20], 0.8); D(9, 3, [200, 200, 30, 31], 0.7)
    # 10: equal scores -- the earlier detection (IoU 0.6) is ranked first and takes the box, the later (IoU 0.9) stays unmatched
    G(10, 3, [0, 0, 10, 10]); D(10, 3, [0, 0, 10, 6], 0.5); D(10, 3, [0, 0, 10, 9], 0.5)
    # 11: an ignored non-crowd box that is matched once and then skipped
    G(11, 3, [0, 0, 50, 50], ign=1); D(11, 3, [0, 0, 50, 49], 0.9); D(11, 3, [0, 0, 50, 48], 0.8)
    # category 5: every box ignored (flag or crowd), with detections on them
    G(0, 5, [0, 0, 30, 30], ign=1); G(1, 5, [0, 0, 60, 60], crowd=1); D(0, 5, [0, 0, 30, 29], 0.9); D(1, 5, [5, 5, 20, 20], 0.8)
    D(2, 5, [0, 0, 10, 10], 0.7)
    return pack_gt(gts), pack_dt(dts), 6, 12


def make_sets():
    return {'small': seeded_set(11, 40, 5, 5.0), 'large': seeded_set(12, 300, 80, 7.5), 'hand': hand_set()}


_CACHE = {}


def load_golden():
    """{set: (gt, dt, K, I, results)} from the committed file"""
    if not _CACHE:
        z = np.load(GOLDEN)
        for s in SETS:
            gt = {k: z['%s_in_gt_%s' % (s, k)] for k in GT_KEYS}
            dt = {k: z['%s_in_dt_%s' % (s, k)] for k in DT_KEYS}
            K, I = (int(v) for v in z['%s_shape' % s])
            res = {k: z['%s_%s' % (s, k)] for k in RESULT_KEYS}
            res['precision'] = np.ascontiguousarray(res['precision'].transpose(0, 4, 1, 2, 3))     # stored (T,K,A,M,R)
            _CACHE[s] = (gt, dt, K, I, res)
    return _CACHE


# ---- further seeded sets ----------------------------------------------------------------------------
SIZES = (0, 1, 2, 63, 64, 65, 100, 101, 130)          # detections and boxes per problem (wave seams 64, maxDets[-1] = 100, beyond it)


def size_grid_set(seed, pairs):
    """one image per (D, G) pair, one category: exactly D detections and G boxes in that problem (a (0, 0) pair is no problem)"""
    parts = [seeded_set(seed + 7 * n, 1, 1, 0, dets_per_problem=dg) for n, dg in enumerate(pairs)]
    gt = {k: np.concatenate([p[0][k] for p in parts]) for k in GT_KEYS}
    dt = {k: np.concatenate([p[1][k] for p in parts]) for k in DT_KEYS}
    gt['image'] = np.concatenate([np.full(len(p[0]['image']), n, np.int32) for n, p in enumerate(parts)])
    dt['image'] = np.concatenate([np.full(len(p[1]['image']), n, np.int32) for n, p in enumerate(parts)])
    return gt, dt, 1, len(pairs)


# The launch arithmetic of sn_coco_accumulate, restated (coco_eval.hip): the ordering launch gives every category
# ceil(N_k / SORT_TILE) workgroups of SORT_TILE detections, the scans walk a category in chunks of SCAN_CHUNK with a carry, and the
# workspace is five 256-byte aligned pieces.  tests/test_gpu_coco_eval.py pins the constants through sn_coco_limits and the layout
# through sn_coco_accumulate_workspace_bytes.
SORT_TILE, SCAN_CHUNK = 256, 256


def workspace_bytes(NK, T, A):
    al = lambda n: (n + 255) // 256 * 256
    n = max(NK, 1)
    return al(8 * n) + al(4 * n) + al(4 * n) + al(4 * A * T * n) + al(8 * A * T * n)


def seam_counts():
    """kept detections per category on both sides of every block seam up to three blocks, plus 0, 1 and about 5 000"""
    out = {0, 1, 5003}
    for tile in (SORT_TILE, SCAN_CHUNK):
        for m in (1, 2, 3):
            out.update((m * tile - 1, m * tile, m * tile + 1))
    return sorted(out)


def category_count_set(seed, counts):
    """category k gets counts[k] detections in all, at most 97 per (image, category) problem (under maxDets[-1] = 100: all are
    kept), one or two boxes per problem, scores quantised to 1/50 (ties across every seam)"""
    rng = np.random.RandomState(seed)
    gts, dts = [], []
    n_img = max(1, max((c + 96) // 97 for c in counts))
    for k, c in enumerate(counts):
        left = c
        for i in range(n_img):
            boxes = []
            for _ in range(1 + (i + k) % 2):
                w, h = np.exp(rng.uniform(np.log(8), np.log(300), 2))
                x, y = rng.uniform(0, 500, 2)
                b = [round(float(v), 2) for v in (x, y, w, h)]
                boxes.append(b)
                gts.append((i, k, b, round(b[2] * b[3] * 0.8, 1), int(rng.rand() < 0.1), 0))
            n = min(left, 97)
            left -= n
            for _ in range(n):
                b = boxes[rng.randint(len(boxes))]
                s = 0.2
                d = [round(float(b[0] + rng.uniform(-s, s) * b[2]), 1), round(float(b[1] + rng.uniform(-s, s) * b[3]), 1),
                     round(float(b[2] * np.exp(rng.uniform(-s, s))), 1), round(float(b[3] * np.exp(rng.uniform(-s, s))), 1)]
                dts.append((i, k, d, round(float(rng.randint(1, 51)) / 50, 8), d[2] * d[3]))
        assert left == 0
    return pack_gt(gts), pack_dt(dts), len(counts), n_img


def all_boxes_of(dt, K, I):
    """a set's detections (xywh) as all_boxes[class][image] = (n,5) float64 rows x1, y1, x2 = x + w - 1, y2 = y + h - 1, score"""
    out = [[np.zeros((0, 5)) for _ in range(I)] for _ in range(K + 1)]
    b = dt['bbox']
    rows = np.stack((b[:, 0], b[:, 1], b[:, 0] + b[:, 2] - 1, b[:, 1] + b[:, 3] - 1, dt['score']), axis=1)
    key = dt['category'].astype(np.int64) * I + dt['image']
    for kk in np.unique(key):
        out[int(kk // I) + 1][int(kk % I)] = rows[key == kk]
    return out


# ---- the device, at the C ABI, with every operand in a guarded buffer ---------------------------------
GUARD = 256          # bytes before and after every operand
FILL = 0x5A


class Guarded(object):
    """device operands with GUARD bytes of FILL on both sides; check() -> the pads are untouched and the inputs unchanged"""

    def __init__(self):
        self.items = []

    def _alloc(self, nbytes):
        import torch
        raw = torch.full((2 * GUARD + max(nbytes, 8),), FILL, dtype=torch.uint8, device='cuda:0')
        return raw

    def put(self, arr):
        import torch
        arr = np.ascontiguousarray(arr)
        raw = self._alloc(arr.nbytes)
        if arr.nbytes:
            raw[GUARD:GUARD + arr.nbytes] = torch.from_numpy(arr.reshape(-1).view(np.uint8).copy()).to('cuda:0')
        self.items.append((raw, arr.nbytes, arr.reshape(-1).view(np.uint8).copy()))
        return raw[GUARD:]

    def out(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        raw = self._alloc(nbytes)
        self.items.append((raw, nbytes, None))
        return raw[GUARD:]

    def check(self):
        for raw, nbytes, want in self.items:
            h = raw.cpu().numpy()
            assert (h[:GUARD] == FILL).all(), 'bytes before an operand were written'
            assert (h[GUARD + nbytes:] == FILL).all(), 'bytes after an operand were written'
            if want is not None:
                assert np.array_equal(h[GUARD:GUARD + nbytes], want), 'an input was modified'

    @staticmethod
    def read(view, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return view[:nbytes].cpu().numpy().view(dtype).reshape(shape).copy()


def device_run(gt, dt, K, params, ev):
    """sn_coco_match + sn_coco_accumulate on the CSR layout `ev` (the restatement's offsets and permutations) -> the arrays named in
    RESULT_KEYS except stats; every operand guarded, the guards checked"""
    import torch
    from sniper_amd import hip
    dp, gp = ev['dt_perm'], ev['gt_perm']
    dt6 = np.concatenate((dt['bbox'][dp], dt['score'][dp, None], dt['area'][dp, None]), axis=1).astype(np.float64).reshape(-1, 6)
    gt5 = np.concatenate((gt['bbox'][gp], gt['area'][gp, None]), axis=1).astype(np.float64).reshape(-1, 5)
    flags = ((gt['iscrowd'][gp] != 0).astype(np.uint8) | ((gt['ignore'][gp] != 0).astype(np.uint8) << 1))
    iou, rec = np.asarray(params.iouThrs, np.float64), np.asarray(params.recThrs, np.float64)
    rng = np.asarray(params.areaRng, np.float64).reshape(-1, 2)
    max_dets = np.asarray(params.maxDets, np.int32)
    T, R, A, M = len(iou), len(rec), len(rng), len(max_dets)
    P, NK, NG = len(ev['prob_cat']), int(ev['kp_off'][-1]), len(gp)
    assert P >= 1
    dcount, gcount = np.diff(ev['dt_off']), np.diff(ev['gt_off'])
    kept_per_cat = np.diff(ev['kp_off'][ev['cat_off']].astype(np.int64))
    G = Guarded()
    d_dt, d_gt, d_flags = G.put(dt6), G.put(gt5), G.put(flags)
    d_dt_off, d_gt_off, d_kp_off, d_cat_off = (G.put(ev[k].astype(np.int32)) for k in ('dt_off', 'gt_off', 'kp_off', 'cat_off'))
    d_iou, d_rec, d_rng = G.put(iou), G.put(rec), G.put(rng)
    o_rank, o_dtm, o_dtig = G.out((NK,), np.int32), G.out((A, T, NK), np.int32), G.out((A, T, NK), np.uint8)
    o_gtm, o_gtig = G.out((A, T, NG), np.int32), G.out((A, NG), np.uint8)
    o_pr, o_rc = G.out((T, R, K, A, M), np.float64), G.out((T, K, A, M), np.float64)
    need = int(hip.query('sn_coco_accumulate_workspace_bytes', NK, T, A))
    assert need == workspace_bytes(NK, T, A)
    ws = G.out((need,), np.uint8)
    hip.call('sn_coco_match', d_dt, d_dt_off, d_kp_off, d_gt, d_flags, d_gt_off, d_iou, d_rng, P, T, A, int(max_dets[-1]),
             int(dcount.max()), int(gcount.max()), NK, NG, o_rank, o_dtm, o_dtig, o_gtm, o_gtig, hip.stream())
    hip.call('sn_coco_accumulate', d_dt, d_dt_off, d_kp_off, d_gt_off, d_cat_off, o_rank, o_dtm, o_dtig, o_gtig, d_rec, max_dets, P, K,
             T, A, M, R, int(max_dets[-1]), int(kept_per_cat.max()), NK, NG, ws, need, o_pr, o_rc, hip.stream())
    torch.cuda.synchronize()
    G.check()
    rd = Guarded.read
    return {'dt_rank': rd(o_rank, (NK,), np.int32), 'dt_match': rd(o_dtm, (A, T, NK), np.int32), 'dt_ignore': rd(o_dtig, (A, T, NK), np.uint8),
            'gt_match': rd(o_gtm, (A, T, NG), np.int32), 'gt_ignore': rd(o_gtig, (A, NG), np.uint8),
            'precision': rd(o_pr, (T, R, K, A, M), np.float64), 'recall': rd(o_rc, (T, K, A, M), np.float64)}


DEVICE_KEYS = ('dt_rank', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore', 'precision', 'recall')


def assert_same_bits(got, want, keys=DEVICE_KEYS, what=''):
    for k in keys:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            bad = np.argwhere(a != b)
            raise AssertionError('%s %s: %d of %d entries differ, first at %s: got %r want %r' % (
                what, k, len(bad), a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))
