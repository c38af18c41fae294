"""-m gpu: sn_voc_match / sn_voc_accumulate and sniper_amd.evaluation's VOC half against the reference's goldens
(tests/golden/voceval_v1.npz: rec, prec and the 11-point AP on the bits, the area AP within the rounding of its sum) and, for what
voc_eval does not return (tp, fp, the order, npos, the match arrays) and where no golden exists, against the restatement
tests/voc_eval_ref.py that the goldens pin -- on the bits.  Every operand of the C-ABI runs sits between guard bytes
(tests/coco_eval_util.py::Guarded) and two runs must give identical bytes.

The area AP's tolerance is derived, not tuned: its terms (mrec[i+1] - mrec[i]) * mpre[i+1] are >= 0 and every partial sum is <= 1, so
any summation order errs by at most (n - 1) * 2^-53 for n terms; numpy's pairwise order and the device's may differ by twice that."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import voc_eval_ref as ref  # noqa: E402
import voc_eval_util as U  # noqa: E402


def _check(gt, dt, K, thresholds, what, want=None, golden=None):
    """device == restatement `want` (computed here unless given) on every exact key, == `golden` where one exists, the area AP within
    its bound of the golden (else of the restatement); two runs identical"""
    if want is None:
        want = ref.run(gt, dt, K, thresholds)
    got = U.device_run(gt, dt['rows'], K, thresholds, want)
    U.assert_same_bits(got, want, keys=U.EXACT_KEYS, what=what)
    truth = golden if golden is not None else want
    if golden is not None:
        U.assert_same_bits(got, golden, keys=('rec', 'prec', 'ap07'), what=what + ' (golden)')
    U.assert_area_within_bound(got['ap_area'], truth['ap_area'], U.recall_changes(truth['rec'], want['cls_off']), what)
    again = U.device_run(gt, dt['rows'], K, thresholds, want)
    for k in U.DEVICE_KEYS:
        assert got[k].tobytes() == again[k].tobytes(), (what, k, 'two runs differ')
    return got


@pytest.mark.parametrize('name', U.SETS)
def test_device_equals_the_reference_goldens(name):
    gt, dt, K, I, golden = U.load_golden()[name]
    got = _check(gt, U.with_rows(dt, golden['rows']), K, U.THRESHOLDS, name, golden=golden)
    assert got['dt_tp'].any() and got['dt_fp'].any()


def _limits():
    from sniper_amd import hip
    out = (ctypes.c_int32 * 5)()
    hip.lib().call('sn_voc_limits', out)
    return list(out)


@pytest.fixture(scope='module')
def size_grid():
    """every (D, G) pair in one call at SN_VOC_MAX_T thresholds; the restatement is computed once and its first threshold serves the
    T = 1 run"""
    max_t = _limits()[2]
    pairs = [(d, g) for d in U.SIZES_D for g in U.SIZES_G]
    gt, dt, K, I = U.size_grid_set(100, pairs)
    dt = U.with_rows(dt)
    thresholds = tuple(np.linspace(0.3, 0.9, max_t))
    return gt, dt, K, thresholds, ref.run(gt, dt, K, thresholds)


def test_every_problem_size_at_the_most_thresholds(size_grid):
    gt, dt, K, thresholds, want = size_grid
    assert len(thresholds) >= 8 and np.diff(want['dt_off']).max() == 1024 and np.diff(want['gt_off']).max() == 256
    got = _check(gt, dt, K, thresholds, 'sizes T = max', want=want)
    assert (got['dt_tp'].sum(axis=1) > 0).all() and (np.diff(got['dt_tp'].sum(axis=1).astype(int)) <= 0).all()


def test_every_problem_size_at_one_threshold(size_grid):
    gt, dt, K, thresholds, full = size_grid
    one = dict(full)
    for k in ('dt_tp', 'dt_fp', 'gt_det', 'rec', 'prec', 'ap07', 'ap_area'):
        one[k] = np.ascontiguousarray(full[k][:1])
    _check(gt, dt, K, thresholds[:1], 'sizes T = 1', want=one)


def test_per_class_counts_across_every_tile_and_chunk_seam():
    tile, chunk = _limits()[3:]
    counts = U.seam_counts(tile, chunk)
    assert counts == [1, tile - 1, tile, tile + 1, 2 * tile + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 5]
    counts = counts[:3] + [0] + counts[3:]                  # an empty class between two full ones
    gt, dt, K, I = U.class_count_set(300, counts)
    got = _check(gt, U.with_rows(dt), K, U.THRESHOLDS, 'seams')
    assert np.array_equal(np.diff(ref.layout(gt, dt, K)['cls_off']), counts)
    assert (got['ap07'][:, 3] == 0).all() and (got['ap_area'][:, 3] == 0).all() and got['npos'][3] == 0
    assert (got['ap07'][0, [1, 2, 4, 5, 6, 7, 8, 9]] > 0).all()


def test_the_tie_rule_is_arrival_order():
    gt, dt, K, I = U.tie_set()
    dt = U.with_rows(dt)
    assert (dt['rows'][dt['category'] == 0, 4] == 0.123).sum() >= 8           # 0.1231 and 0.1234: equal only after the rounding
    want = ref.run(gt, dt, K)
    got = _check(gt, dt, K, U.THRESHOLDS, 'ties', want=want)
    wrong = ref.run(gt, dt, K, defect='unstable_ties')
    assert not U.same_bits(got['order'], wrong['order']) and not U.same_bits(got['prec'], wrong['prec'])


def test_boxes_submitted_as_detections_score_one():
    gt, _, K, I = U.seeded_set(51, 30, 4, 4.0, lambda i, rng: 0)
    gt = dict(gt, difficult=np.zeros_like(gt['difficult']))
    n = len(gt['image'])
    o = np.argsort(gt['category'].astype(np.int64) * I + gt['image'], kind='stable')
    raw = np.concatenate((gt['bbox'][o] - 1, np.zeros((n, 1))), axis=1).astype(np.float32)
    dt = {'image': gt['image'][o], 'category': gt['category'][o], 'raw': raw}
    rs = np.random.RandomState(2)
    for k in range(K):
        sel = np.flatnonzero(dt['category'] == k)
        assert len(sel) >= 3
        dt['raw'][sel, 4] = U._distinct_scores(rs, len(sel))
    dt = U.with_rows(dt)
    got = _check(gt, dt, K, U.THRESHOLDS, 'boxes as detections')
    cls_off = ref.layout(gt, dt, K)['cls_off']
    n_terms = U.recall_changes(got['rec'], cls_off)
    assert np.array_equal(n_terms, np.broadcast_to(np.diff(cls_off), n_terms.shape))
    one = np.ones_like(got['ap07'])
    U.assert_area_within_bound(got['ap07'], one, n_terms, 'ap07 = 1')
    U.assert_area_within_bound(got['ap_area'], one, n_terms, 'ap_area = 1')
    assert (got['rec'][:, cls_off[1:] - 1] == 1.0).all() and (got['prec'] == 1.0).all() and got['dt_tp'].all()


def test_evaluator_equals_the_restatement_and_the_goldens():
    """the public interface on a golden set: all_boxes -> the rows of the result file -> CSR -> both kernels -> the summary"""
    from sniper_amd.evaluation import VOCBoxEvaluator
    gt, dt, K, I, golden = U.load_golden()['voc_like']
    names = ['class%02d' % k for k in range(K)]
    want = ref.run(gt, U.with_rows(dt, golden['rows']), K)
    for use07 in (True, False):
        ev = VOCBoxEvaluator(gt, I, names, use07)
        res = ev.evaluate(U.all_boxes_of(dt, K, I), return_curves=True)
        assert U.same_bits(res.ap07, golden['ap07']) and U.same_bits(res.curves['rec'], golden['rec']) and U.same_bits(res.curves['prec'], golden['prec'])
        U.assert_area_within_bound(res.ap_area, golden['ap_area'], U.recall_changes(golden['rec'], golden['cls_off']), 'evaluator')
        U.assert_same_bits(res.curves, want, keys=('dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det', 'order'), what='evaluator')
        assert np.array_equal(res.npos, want['npos']) and res.ap is (res.ap07 if use07 else res.ap_area)
        assert res.summary() == ref.summary(res.ap, names, use07) and len(res.summary().split('\n')) == 2 * (K + 1) + 2
        rec, prec = res.curve(1, 3)
        assert U.same_bits(rec, golden['rec'][1, golden['cls_off'][3]:golden['cls_off'][4]]) and len(prec) == len(rec)
        assert set(res.timing) == {'host_s', 'upload_s', 'kernels_s', 'match_s', 'accumulate_s', 'download_s', 'problems', 'detections', 'kept', 'boxes'}
    assert 0.2 < res.mean_ap[1] < res.mean_ap[0] < 0.9
    empty = VOCBoxEvaluator({k: v[:0] for k, v in gt.items()}, I, names, True).evaluate([[[] for _ in range(I)] for _ in range(K + 1)])
    assert (empty.ap == 0).all() and (empty.npos == 0).all()


def test_inference_detections_through_aggregate_into_evaluate_detections_voc():
    """end to end: the small two-scale inference set-up of tests/test_gpu_inference.py -> Tester.aggregate (inside
    imdb_detection_wrapper) -> evaluate_detections_voc, compared with the restatement on the same rows"""
    import sniper_amd.mx as mx
    from sniper_amd import config as cfgmod
    from sniper_amd import inference
    from sniper_amd.evaluation import VOCBoxEvaluator, evaluate_detections_voc
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
    assert sum(len(d) for per in all_boxes[1:] for d in per) > 0
    # ground truth: every third detection's box (so that something matches; every fifth of those difficult), plus a box nothing detects
    for i, r in enumerate(roidb):
        boxes, classes = [], []
        for c in range(1, 81):
            for row in np.asarray(all_boxes[c][i], np.float64).reshape(-1, 5)[::3]:
                boxes.append(np.round(row[:4]))
                classes.append(c)
        boxes.append([1., 2., 30., 40.]); classes.append(80)
        boxes.append([0., 0., 0., 0.]); classes.append(0)                 # a proposal row: not ground truth
        r['boxes'], r['gt_classes'] = np.array(boxes, np.float32), np.array(classes, np.int32)
        r['gt_difficult'] = (np.arange(len(classes)) % 5 == 4).astype(np.int32)
    res = evaluate_detections_voc(all_boxes, roidb, 81)
    ev = VOCBoxEvaluator.from_roidb(roidb, 81)
    rows, counts = ev.convert_detections(all_boxes)
    kk, ii = np.nonzero(counts)
    dt = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'rows': rows}
    gt = dict(ev.gt, difficult=ev.gt['difficult'].astype(np.int32))
    want = ref.run(gt, dt, 80)
    assert U.same_bits(res.ap07, want['ap07']) and np.array_equal(res.npos, want['npos']) and res.use_07_metric and res.ap is res.ap07
    U.assert_area_within_bound(res.ap_area, want['ap_area'], U.recall_changes(want['rec'], want['cls_off']), 'end to end')
    assert res.mean_ap[0] > 0 and res.summary() == ref.summary(want['ap07'], ev.class_names, True)
    assert len(res.summary().split('\n')) == 1 + 81 + 1 + 81 and res.summary().startswith('VOC07 metric? Y\nAP for class1 = ')
