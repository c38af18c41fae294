"""-m gpu: sn_rle_stats / sn_rle_iou / sn_coco_match_iou and sniper_amd.evaluation.COCOSegmEvaluator against the reference's goldens
(tests/golden/cocosegm_v1.npz) stage by stage, and against the plain-Python restatement (tests/coco_segm_ref.py) on a grid of
problem sizes and run counts that crosses every seam sn_rle_limits reports.  Every operand sits between guard bytes, two runs give
the same bytes, and there is no tolerance anywhere: counts are integers, an IoU is one float64 division of two integers."""
import ctypes

import numpy as np
import pytest

import coco_segm_ref as ref
import coco_segm_util as U
from coco_eval_util import DEVICE_KEYS, assert_same_bits

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 130)          # detections and annotations per problem: the wave seams and beyond maxDets[-1] = 100


@pytest.fixture(scope='module')
def golden():
    return U.load_golden()


@pytest.fixture(scope='module')
def limits():
    from sniper_amd import hip
    out = (ctypes.c_int32 * 5)()
    hip.lib().call('sn_rle_limits', out)
    return dict(zip(('max_dt', 'max_gt', 'wave', 'per_group', 'threads'), (int(v) for v in out)))


def test_limits(limits):
    assert limits == {'max_dt': 1024, 'max_gt': 256, 'wave': 64, 'per_group': 4, 'threads': 256}


def _cum2(rles):
    """what sn_rle_stats keeps per run: its end position and the 1-pixels up to and including it"""
    out = []
    for r in rles:
        r = np.asarray(r, np.int64)
        ones = np.where(np.arange(len(r)) % 2 == 1, r, 0)
        out.append(np.stack((np.cumsum(r), np.cumsum(ones)), axis=1))
    return (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.uint32)


# ---- the goldens, stage by stage ----------------------------------------------------------------------
@pytest.mark.parametrize('s', U.SETS)
def test_golden_stages(golden, s):
    d = golden[s]
    gt, dt = U.ref_inputs(d)
    rows, cum = U.device_stats(d['dt_counts'], dt['hw'], d['dt_score'])
    assert rows[:, :4].tobytes() == d['dt_bbox'].tobytes(), 'rleToBbox'
    assert rows[:, 5].tobytes() == d['dt_area'].tobytes() and rows[:, 4].tobytes() == d['dt_score'].tobytes(), 'rleArea / score'
    assert np.array_equal(cum, _cum2(d['dt_counts']))
    ev = ref.evaluate(gt, dt, d['K'])               # the CSR layout (offsets and permutations) the C ABI takes
    iou, iou_off, d_rows, g_rows = U.device_iou(ev, gt, dt)
    assert np.array_equal(iou_off, d['iou_off']) and iou.tobytes() == d['iou'].tobytes(), 'rleIou'
    assert np.array_equal(d_rows, rows[ev['dt_perm']])
    got = U.device_match(ev, gt, d_rows, iou, iou_off, d['K'], ref.Params())
    assert_same_bits(got, d['res'], what=s)
    again = U.device_match(ev, gt, d_rows, U.device_iou(ev, gt, dt)[0], iou_off, d['K'], ref.Params())
    assert_same_bits(again, got, what=s + ' second run')


def test_the_column_wrap_pair(golden):
    """h = w = 10, ground truth [35, 8, 57] against detection [40, 2, 58]: two common pixels, and the reference says 0"""
    gt = {'image': np.zeros(1, np.int32), 'category': np.zeros(1, np.int32), 'area': np.array([8.]), 'iscrowd': np.zeros(1, np.int32),
          'ignore': np.zeros(1, np.int32), 'rle': [np.array(U.QUIRK_GT, np.uint32)], 'hw': np.array([[10, 10]], np.int32)}
    dt = {'image': np.zeros(1, np.int32), 'category': np.zeros(1, np.int32), 'score': np.array([.5]), 'rle': [np.array(U.QUIRK_DT, np.uint32)],
          'hw': np.array([[10, 10]], np.int32)}
    ev = ref.evaluate(gt, dt, 1)
    iou, _, d_rows, g_rows = U.device_iou(ev, gt, dt)
    assert iou.tolist() == [0.0]
    assert d_rows[0, :4].tolist() == [4., 0., 1., 2.] and g_rows[0, :4].tolist() == [3., 2., 2., 4.] and d_rows[0, 5] == 2.
    # the same counts in a 50 x 2 image lie in one column, nothing wraps, and the common pixels count
    gt['hw'] = dt['hw'] = np.array([[50, 2]], np.int32)
    assert U.device_iou(ev, gt, dt)[0].tolist() == [2. / 8.]


# ---- the Python surface ---------------------------------------------------------------------------------
@pytest.mark.parametrize('s', U.SETS)
def test_evaluator_matches_the_golden(golden, s):
    from sniper_amd.evaluation import COCOSegmEvaluator, COCOSegmResult
    d = golden[s]
    boxes, masks = U.detections_of(d)
    args = (U.gt_dict(d, polygons=False), range(1, d['I'] + 1), range(1, d['K'] + 1), d['sizes'])
    res = COCOSegmEvaluator(*args).evaluate(boxes, masks, return_matches=True, return_rles=True)
    want = d['res']
    assert isinstance(res, COCOSegmResult)
    assert res.precision.tobytes() == want['precision'].tobytes() and res.recall.tobytes() == want['recall'].tobytes()
    assert res.stats.tobytes() == want['stats'].tobytes()
    assert res.matches['iou'].tobytes() == d['iou'].tobytes() and np.array_equal(res.matches['iou_off'], d['iou_off'])
    assert_same_bits(res.matches, want, keys=('dt_rank', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore'), what=s)
    lines = res.summary().split('\n')
    assert len(lines) == 12 and lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %.3f' % want['stats'][0]
    assert res.timing['chunks'] == 1 and all(k in res.timing for k in ('host_s', 'upload_s', 'stats_s', 'iou_s', 'match_s', 'accumulate_s', 'download_s'))
    assert len(res.rles['dt']) == len(d['dt_counts']) and len(res.rles['gt']) == len(d['gt_counts'])
    # the same in chunks of a few problems each: the problems of a chunk are a slice of the offsets
    small = COCOSegmEvaluator(*args, chunk_elements=300).evaluate(boxes, masks, return_matches=True)
    assert small.timing['chunks'] > 2 or s != 'seeded'
    assert small.precision.tobytes() == res.precision.tobytes() and small.recall.tobytes() == res.recall.tobytes()
    assert small.matches['iou'].tobytes() == res.matches['iou'].tobytes()
    assert_same_bits(small.matches, res.matches, keys=('dt_rank', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore'), what=s + ' chunked')


def test_evaluator_without_anything(golden):
    from sniper_amd.evaluation import COCOSegmEvaluator
    d = golden['hand']
    gt = {k: [] for k in ('image', 'category', 'area', 'iscrowd', 'segmentation')}
    boxes = [[np.zeros((0, 5)) for _ in range(d['I'])] for _ in range(d['K'] + 1)]
    masks = [[[] for _ in range(d['I'])] for _ in range(d['K'] + 1)]
    res = COCOSegmEvaluator(gt, range(d['I']), range(d['K']), d['sizes']).evaluate(boxes, masks)
    assert (res.precision == -1).all() and (res.stats == -1).all()
    # detections only: every category lacks ground truth, the matching still runs
    boxes, masks = U.detections_of(d)
    res = COCOSegmEvaluator(gt, range(d['I']), range(d['K']), d['sizes']).evaluate(boxes, masks)
    assert (res.precision == -1).all()


# ---- the size grid against the restatement ----------------------------------------------------------------
def _mask_with_runs(rng, m, h, w):
    """counts of exactly m runs (m >= 1) that sum to h * w; the first count is 0 in half of the masks with m >= 2"""
    total = h * w
    lead0 = m >= 2 and rng.rand() < 0.5
    k = m - 1 if lead0 else m
    assert 1 <= k <= total
    cuts = np.sort(rng.choice(np.arange(1, total), size=k - 1, replace=False)) if k > 1 else np.zeros(0, np.int64)
    c = np.diff(np.concatenate([[0], cuts, [total]]))
    return np.concatenate([[0], c]).astype(np.uint32) if lead0 else c.astype(np.uint32)


def _grid_set(limits, seed=5):
    """one category, one image per (D, G) pair of SIZES x SIZES, image 24 x 40 = 960 pixels.  Most masks are a rectangle (3 or 4
    runs per column it spans... a few dozen runs); the first masks of every problem get the run counts that cross the seams of the
    scan (a wave of runs) and of the search (a wave of 1-runs = two waves of runs): 1, 2, 3, wave - 1 .. 2 * wave + 1, 4 * wave + 2"""
    rng = np.random.RandomState(seed)
    wv = limits['wave']
    runs = [1, 2, 3, wv - 1, wv, wv + 1, 2 * wv - 1, 2 * wv, 2 * wv + 1, 2 * wv + 2, 2 * wv + 3, 4 * wv + 2]
    h, w = 24, 40
    sizes, gt, dt = [], {k: [] for k in ('image', 'category', 'area', 'iscrowd', 'ignore', 'rle')}, {k: [] for k in ('image', 'category', 'score', 'rle')}

    def blob(n):
        if n < len(runs):
            return _mask_with_runs(rng, runs[n], h, w)
        y0, x0 = rng.randint(h - 4), rng.randint(w - 4)
        m = np.zeros((h, w), np.uint8)
        m[y0:y0 + rng.randint(2, 12), x0:x0 + rng.randint(2, 12)] = 1
        return ref.rle_encode(m)
    for D in SIZES:
        for G in SIZES:
            if D == 0 and G == 0:
                continue
            i = len(sizes)
            sizes.append((h, w))
            for n in range(G):
                r = blob(n)
                gt['image'].append(i), gt['category'].append(0), gt['rle'].append(r)
                gt['area'].append(float(ref.rle_area(r)) * (1, 1, 4, 12)[rng.randint(4)])
                gt['iscrowd'].append(int(rng.rand() < 0.15)), gt['ignore'].append(int(rng.rand() < 0.05))
            for n in range(D):
                src = gt['rle'][-1 - rng.randint(G)] if G and rng.rand() < 0.5 else None
                r = blob(n) if src is None or n < len(runs) else src          # half of the plain detections copy an annotation: IoU 1
                dt['image'].append(i), dt['category'].append(0), dt['rle'].append(r)
                dt['score'].append(round(float(rng.randint(1, 51)) / 50, 8))
    sizes = np.array(sizes, np.int32)
    gt = {k: (v if k == 'rle' else np.array(v, np.float64 if k == 'area' else np.int32)) for k, v in gt.items()}
    dt = {k: (v if k == 'rle' else np.array(v, np.float64 if k == 'score' else np.int32)) for k, v in dt.items()}
    gt['hw'], dt['hw'] = sizes[gt['image']].reshape(-1, 2), sizes[dt['image']].reshape(-1, 2)
    return gt, dt, sizes


@pytest.fixture(scope='module')
def grid(limits):
    gt, dt, sizes = _grid_set(limits)
    cache = {}
    wide = ref.Params()
    wide.maxDets = [3, 130]
    return gt, dt, sizes, ref.run(gt, dt, 1, cache=cache), ref.run(gt, dt, 1, wide, summary=False, cache=cache), wide


def test_grid_stats_and_iou(grid):
    gt, dt, sizes, want, _, _ = grid
    rows, cum = U.device_stats(dt['rle'], dt['hw'], dt['score'])
    assert rows.tobytes() == ref.stats_rows(dt['rle'], dt['hw'], dt['score']).tobytes()
    assert np.array_equal(cum, _cum2(dt['rle']))
    g_rows, g_cum = U.device_stats(gt['rle'], gt['hw'])
    assert g_rows.tobytes() == ref.stats_rows(gt['rle'], gt['hw']).tobytes() and np.array_equal(g_cum, _cum2(gt['rle']))
    iou, iou_off, _, _ = U.device_iou(want, gt, dt)
    assert np.array_equal(iou_off, want['iou_off'])
    assert iou.tobytes() == want['iou'].tobytes()
    assert ((iou > 0) & (iou < 1)).sum() > 1000 and (iou == 1).sum() > 100 and (iou == 0).sum() > 1000
    assert U.device_iou(want, gt, dt)[0].tobytes() == iou.tobytes(), 'second run'


@pytest.mark.parametrize('which', ('default', 'wide'))
def test_grid_matches(grid, which):
    gt, dt, sizes, default, wide, wide_params = grid
    want, params = (default, ref.Params()) if which == 'default' else (wide, wide_params)
    rows = ref.stats_rows([dt['rle'][n] for n in want['dt_perm']], dt['hw'][want['dt_perm']], dt['score'][want['dt_perm']])
    got = U.device_match(want, gt, rows, want['iou'], want['iou_off'], 1, params)
    assert_same_bits(got, want, keys=DEVICE_KEYS, what=which)
    assert (got['dt_match'] != 0).any() and (got['dt_match'] == 0).any() and got['dt_ignore'].any() and got['gt_ignore'].any()


def test_grid_through_the_evaluator(grid):
    from sniper_amd.evaluation import COCOSegmEvaluator
    gt, dt, sizes, want, _, _ = grid
    I = len(sizes)
    boxes = [[np.zeros((0, 5))] * I, [np.zeros((0, 5))] * I]
    masks = [[[]] * I, [[] for _ in range(I)]]
    for n in range(len(dt['image'])):
        i = int(dt['image'][n])
        boxes[1][i] = np.concatenate((boxes[1][i], [[0, 0, 0, 0, dt['score'][n]]]))
        masks[1][i].append({'size': [24, 40], 'counts': dt['rle'][n]})
    g = dict(gt, segmentation=[{'size': [24, 40], 'counts': r} for r in gt['rle']])
    res = COCOSegmEvaluator(g, range(I), [1], sizes, chunk_elements=20000).evaluate(boxes, masks, return_matches=True)
    assert res.timing['chunks'] > 3
    assert res.precision.tobytes() == want['precision'].tobytes() and res.recall.tobytes() == want['recall'].tobytes()
    assert res.matches['iou'].tobytes() == want['iou'].tobytes()


def test_problems_over_the_caps_are_refused(limits):
    from sniper_amd.evaluation import COCOSegmEvaluator
    one = {'size': [2, 2], 'counts': [1, 2, 1]}
    for n_dt, n_gt, words in ((limits['max_dt'] + 1, 1, 'a problem has 1025 detections'), (1, limits['max_gt'] + 1, 'a problem has 257 masks of ground truth')):
        gt = {'image': [0] * n_gt, 'category': [0] * n_gt, 'area': [2.] * n_gt, 'iscrowd': [0] * n_gt, 'segmentation': [one] * n_gt}
        boxes = [[np.zeros((0, 5))], [np.tile([[0, 0, 1, 1, .5]], (n_dt, 1))]]
        with pytest.raises(ValueError, match=words):
            COCOSegmEvaluator(gt, [1], [1], [[2, 2]]).evaluate(boxes, [[[]], [[one] * n_dt]])


# ---- the one-call form ------------------------------------------------------------------------------------
@pytest.mark.parametrize('s', U.SETS)
def test_evaluate_sds_prints_the_twelve_numbers(golden, s):
    """a roidb carries no ignore flag: the edge set (which has none) must give the golden's numbers, the other two those of the
    restatement with the flags cleared"""
    from sniper_amd.evaluation import evaluate_sds
    d = golden[s]
    gt, dt = U.ref_inputs(d)
    want = ref.run(dict(gt, ignore=np.zeros_like(gt['ignore'])), dt, d['K'])
    if not d['gt_ignore'].any():
        assert s == 'edge' and want['stats'].tobytes() == d['res']['stats'].tobytes()
    boxes, masks = U.detections_of(d)
    roidb, num_classes = U.roidb_of(d)
    res = evaluate_sds(boxes, masks, roidb, num_classes)
    assert res.stats.tobytes() == want['stats'].tobytes() and res.precision.tobytes() == want['precision'].tobytes()
    assert res.summary().split('\n') == want['summary']
    # without gt_areas the area is the mask's own rleArea, from the device
    roidb, _ = U.roidb_of(d, with_areas=False)
    own = dict(gt, ignore=np.zeros_like(gt['ignore']), area=np.array([ref.rle_area(r) for r in gt['rle']], np.float64))
    res = evaluate_sds(boxes, masks, roidb, num_classes)
    assert res.precision.tobytes() == ref.run(own, dt, d['K'])['precision'].tobytes()
