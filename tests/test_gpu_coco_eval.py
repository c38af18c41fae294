"""-m gpu: sn_coco_match / sn_coco_accumulate and sniper_amd.evaluation against the reference's goldens (tests/golden/cocoeval_v1.npz)
and, where no golden exists, against the restatement tests/coco_eval_ref.py that the goldens pin -- on the bits, no tolerance.  Every
operand of the C-ABI runs sits between guard bytes (tests/coco_eval_util.py::Guarded) and two runs must give identical bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import coco_eval_ref as ref  # noqa: E402
import coco_eval_util as U  # noqa: E402


class _P(ref.Params):
    def __init__(self, thrs=None, rng=None, max_dets=None, rec=None):
        ref.Params.__init__(self)
        if thrs is not None:
            self.iouThrs = np.asarray(thrs, np.float64)
        if rng is not None:
            self.areaRng = rng
        if max_dets is not None:
            self.maxDets = list(max_dets)
        if rec is not None:
            self.recThrs = np.asarray(rec, np.float64)


def _check(gt, dt, K, params, what, want=None):
    if want is None:
        want = ref.run(gt, dt, K, params, summary=False)
    ev = want if 'dt_off' in want else ref.evaluate(gt, dt, K, params)
    got = U.device_run(gt, dt, K, params, ev)
    U.assert_same_bits(got, want, what=what)
    again = U.device_run(gt, dt, K, params, ev)
    for k in U.DEVICE_KEYS:
        assert got[k].tobytes() == again[k].tobytes(), (what, k, 'two runs differ')
    return got


@pytest.mark.parametrize('name', U.SETS)
def test_device_equals_the_reference_goldens(name):
    gt, dt, K, I, want = U.load_golden()[name]
    _check(gt, dt, K, ref.Params(), name, want=dict(want))


def test_limits_and_launch_arithmetic_are_what_the_utility_restates():
    import ctypes
    from sniper_amd import hip
    out = (ctypes.c_int32 * 8)()
    hip.lib().call('sn_coco_limits', out)
    assert list(out)[6:] == [U.SORT_TILE, U.SCAN_CHUNK]
    for NK, T, A in ((0, 1, 1), (1, 10, 4), (257, 3, 2), (5003, 16, 8)):
        assert int(hip.query('sn_coco_accumulate_workspace_bytes', NK, T, A)) == U.workspace_bytes(NK, T, A)


def test_every_problem_size_one_threshold_one_range():
    pairs = [(d, g) for d in U.SIZES for g in U.SIZES]
    gt, dt, K, I = U.size_grid_set(100, pairs)
    _check(gt, dt, K, _P(thrs=[0.5], rng=[[0, 1e10]], max_dets=[100]), 'sizes 1x1')


def test_problem_sizes_ten_thresholds_four_ranges():
    low = (0, 1, 2, 63, 64, 65)
    pairs = [(d, g) for d in low for g in low] + [(130, 130), (100, 101), (101, 100), (130, 2), (2, 130), (100, 1), (101, 2), (130, 63), (63, 130),
                                                        (64, 100), (65, 101)]
    gt, dt, K, I = U.size_grid_set(200, pairs)
    _check(gt, dt, K, ref.Params(), 'sizes 10x4')


def test_single_max_dets_and_custom_thresholds_on_the_small_set():
    gt, dt, K, I, _ = U.load_golden()['small']
    _check(gt, dt, K, _P(max_dets=[100]), 'small [100]')
    _check(gt, dt, K, _P(thrs=[0.5], rng=[[0, 1e10]], max_dets=[1, 10, 100]), 'small 1x1 [1,10,100]')
    # recall thresholds that are not ascending: the reference's loop ends at the first index past the end, whatever follows
    _check(gt, dt, K, _P(thrs=[0.5, 0.9], rng=[[0, 1e10], [0, 1024]], max_dets=[2, 7], rec=[0.0, 0.5, 1.0, 0.25, 0.75]), 'small rec')
    gt, dt, K, I, _ = U.load_golden()['hand']
    _check(gt, dt, K, _P(max_dets=[3, 130]), 'hand [3,130]')          # all 130 detections of the big problem kept


def test_per_category_counts_across_every_block_seam():
    counts = U.seam_counts()
    assert {0, 1, 255, 256, 257, 511, 512, 513, 767, 768, 769, 5003} <= set(counts)
    gt, dt, K, I = U.category_count_set(300, counts)
    got = _check(gt, dt, K, _P(thrs=[0.5, 0.75], rng=[[0, 1e10], [1024, 9216]]), 'seams')
    assert (got['precision'] > 0).any()


def test_evaluator_equals_the_restatement_on_seeded_detections():
    """the public interface: all_boxes -> the reference's rounding -> CSR -> both kernels -> stats"""
    import torch
    from sniper_amd.evaluation import COCOBoxEvaluator
    gt, dt, K, I = U.seeded_set(21, 30, 6, 6.0)
    rs = np.random.RandomState(4)
    all_boxes = U.all_boxes_of(dt, K, I)
    for c in range(1, K + 1):                             # float32 rows with awkward decimals, as a network gives them
        for i in range(I):
            d = all_boxes[c][i]
            all_boxes[c][i] = (d + np.hstack((rs.uniform(-0.3, 0.3, (len(d), 4)), np.zeros((len(d), 1))))).astype(np.float32)
    ev = COCOBoxEvaluator(gt, range(1, I + 1), range(1, K + 1))
    res = ev.evaluate(all_boxes, return_matches=True)
    rows, counts = ev.convert_detections(all_boxes)
    kk, ii = np.nonzero(counts)
    dt2 = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'bbox': rows[:, :4], 'score': rows[:, 4],
           'area': rows[:, 5]}
    want = ref.run(gt, dt2, K)
    assert res.precision.tobytes() == want['precision'].tobytes() and res.recall.tobytes() == want['recall'].tobytes()
    assert res.stats.tobytes() == want['stats'].tobytes() and res.summary().split('\n') == want['summary']
    assert 0.05 < res.stats[0] < 0.95
    U.assert_same_bits(res.matches, want, keys=('dt_rank', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore'), what='evaluator')
    # round_results=False: device-resident rows, no rounding -- the restatement on the unrounded rows
    dev_boxes = [all_boxes[0]] + [[torch.from_numpy(np.asarray(d, np.float32).reshape(-1, 5)).to('cuda:0') for d in per] for per in all_boxes[1:]]
    raw = ev.evaluate(dev_boxes, round_results=False)
    r = np.concatenate([np.asarray(d, np.float64).reshape(-1, 5) for per in all_boxes[1:] for d in per])
    w, h = r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1
    dt3 = dict(dt2, bbox=np.stack((r[:, 0], r[:, 1], w, h), axis=1), score=r[:, 4], area=w * h)
    want3 = ref.run(gt, dt3, K)
    assert raw.precision.tobytes() == want3['precision'].tobytes() and raw.recall.tobytes() == want3['recall'].tobytes()
    host_raw = ev.evaluate(all_boxes, round_results=False)
    assert host_raw.precision.tobytes() == raw.precision.tobytes()
    assert raw.precision.tobytes() != res.precision.tobytes()            # the rounding is not a no-op here


def test_inference_detections_through_aggregate_into_evaluate_detections():
    """end to end: the small two-scale inference set-up of tests/test_gpu_inference.py -> Tester.aggregate (inside
    imdb_detection_wrapper) -> evaluate_detections, compared with the restatement on the same rows"""
    import sniper_amd.mx as mx
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    from sniper_amd.evaluation import COCOBoxEvaluator, evaluate_detections
    from sniper_amd.symbols.faster import resnet_mx_101_e2e as rn
    from test_gpu_inference import _Imdb, _roidb
    rs = np.random.RandomState(5)
    roidb = _roidb(4, rs, sizes=((240, 320),))
    cfg = cfgmod.res101_e2e_autofocus()
    cfg.TEST.SCALES = ((240, 320), (480, 640))
    cfg.TEST.BATCH_IMAGES = (2, 2)
    cfg.TEST.VALID_RANGES = ((40, -1), (-1, 60))
    cfg.TEST.DO_PRUNING = (False, True)
    cfg.TEST.CHIP_HYPERPARAMS = ((3, 0.3, 4), (-1, -1, -1))
    cfg.TEST.MAX_PER_IMAGE = 50
    cfg.TEST.RPN_PRE_NMS_TOP_N, cfg.TEST.RPN_POST_NMS_TOP_N = 500, 100

    def fmap(scale_i, image, chip, net_map):
        out = np.zeros_like(np.asarray(net_map, np.float32))
        out[0] = 1.0
        out[1, 1:3, 1:3] = 0.9
        out[0] -= out[1]
        return out
    all_boxes = inference.imdb_detection_wrapper(rn.resnet_mx_101_e2e, cfg, _Imdb(81), [dict(r) for r in roidb], [mx.gpu(0)], None, None,
                                                 focus_map_fn=fmap, lanes=1)
    n_det = sum(len(d) for per in all_boxes[1:] for d in per)
    assert n_det > 0
    # ground truth: every third detection's box (so that something matches), plus a crowd and a box nothing detects, per image
    for i, r in enumerate(roidb):
        boxes, classes = [], []
        for c in range(1, 81):
            for row in np.asarray(all_boxes[c][i], np.float64).reshape(-1, 5)[::3]:
                boxes.append(np.round(row[:4]))
                classes.append(c)
        boxes.append([5., 5., 200., 150.]); classes.append(1 + i)
        boxes.append([1., 2., 30., 40.]); classes.append(80)
        boxes.append([0., 0., 0., 0.]); classes.append(0)                 # a proposal row: not ground truth
        r['boxes'], r['gt_classes'] = np.array(boxes, np.float32), np.array(classes, np.int32)
        r['gt_iscrowd'] = (np.arange(len(classes)) == len(classes) - 3).astype(np.int32)
    res = evaluate_detections(all_boxes, roidb, 81)
    ev = COCOBoxEvaluator.from_roidb(roidb, 81)
    rows, counts = ev.convert_detections(all_boxes)
    kk, ii = np.nonzero(counts)
    dt = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'bbox': rows[:, :4], 'score': rows[:, 4],
          'area': rows[:, 5]}
    gt = dict(ev.gt, iscrowd=ev.gt['iscrowd'].astype(np.int32), ignore=ev.gt['ignore'].astype(np.int32))
    want = ref.run(gt, dt, 80)
    assert res.precision.tobytes() == want['precision'].tobytes() and res.recall.tobytes() == want['recall'].tobytes()
    assert res.stats.tobytes() == want['stats'].tobytes()
    assert res.stats[0] > 0 and len(res.summary().split('\n')) == 12 and res.per_class_ap.shape == (80,)
