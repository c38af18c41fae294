"""CPU: the PASCAL VOC box evaluation without a device.  tests/golden/voceval_v1.npz was written by the reference's own voc_eval
(tests/golden/make_voceval_golden.py); the restatement tests/voc_eval_ref.py must equal its rec, prec and both APs on the bits (a nan
where the reference has one), each planted misreading of the reference must change at least one of them, and the host side of
sniper_amd.evaluation (the rows of the result file, ground truth from a roidb, the metric rule, the summary) is checked against
the golden's rows and plain Python."""
import numpy as np
import pytest

import voc_eval_ref as ref
import voc_eval_util as U

RESULT_KEYS = ('rec', 'prec', 'ap07', 'ap_area')


def _restate(name, defect=None):
    gt, dt, K, I, want = U.load_golden()[name]
    return ref.run(gt, U.with_rows(dt, want['rows']), K, U.THRESHOLDS, defect=defect)


@pytest.fixture(scope='module')
def restated():
    return {s: _restate(s) for s in U.SETS}


@pytest.mark.parametrize('name', U.SETS)
def test_restatement_equals_the_reference_on_the_bits(restated, name):
    want = U.load_golden()[name][4]
    U.assert_same_bits(restated[name], want, keys=RESULT_KEYS, what=name)
    assert np.array_equal(restated[name]['cls_off'], want['cls_off'])


def test_goldens_hold_what_the_issue_lists(restated):
    g = U.load_golden()
    assert g['small'][2:4] == (3, 40) and g['voc_like'][2:4] == (20, 200)
    counts = np.bincount(g['voc_like'][1]['image'], minlength=200)
    assert counts.max() == 200 and 4000 <= counts.sum() <= 7000
    for name in U.SETS:                               # scores distinct within every class after the rounding: the reference's order is defined
        gt, dt, K, I, want = g[name]
        for k in range(K):
            s = want['rows'][want['cls_off'][k]:want['cls_off'][k + 1], 4]
            assert len(np.unique(s)) == len(s), (name, k)
    gt, dt, K, I, want = g['edges']
    r = restated['edges']
    iou = {(int(dt['image'][n]), int(dt['category'][n]), round(float(want['rows'][n, 4]), 3)): r['dt_iou'][n] for n in range(len(dt['image']))}
    assert iou[0, 0, 0.95] == 0.5 and iou[1, 0, 0.94] == 0.7 and iou[8, 0, 0.35] == 0.5          # exactly at the thresholds
    assert iou[6, 0, 0.5] == -np.inf                                                                  # an image without boxes of the class
    off = want['cls_off']
    assert off[3] == off[2] and r['npos'][2] == 1                                                     # class 2: boxes, no detections
    assert off[4] - off[3] == 3 and r['npos'][3] == 0                                                 # class 3: detections, npos = 0
    assert np.isnan(want['rec'][:, off[3]:off[4]]).all() and np.isnan(want['ap_area'][:, 3]).all() and (want['ap07'][:, 3] == 0).all()
    assert off[5] == off[4] and r['npos'][4] == 0 and (want['ap07'][:, 4] == 0).all() and (want['ap_area'][:, 4] == 0).all()   # neither
    assert off[6] - off[5] == 2 and r['npos'][5] == 0                                                 # class 5: detections, no box at all
    # the first-ranked detection of class 0 sits on a difficult box: prec = 0 / eps = 0 there
    assert want['prec'][0, off[0]] == 0.0 and want['rec'][0, off[0]] == 0.0 and r['dt_tp'][0, r['order'][0]] == 0 and r['dt_fp'][0, r['order'][0]] == 0
    # three claimants of one box: one tp (the highest score), two fp; two identical boxes: the second stays free
    img5 = np.flatnonzero((dt['image'] == 5) & (dt['category'] == 0))
    assert r['dt_tp'][0, img5].tolist() == [0, 1, 0] and r['dt_fp'][0, img5].tolist() == [1, 0, 1]
    g2 = np.flatnonzero((gt['image'][r['gt_perm']] == 2) & (gt['category'][r['gt_perm']] == 0))
    assert r['gt_det'][0, g2].tolist() == [1, 0]


@pytest.mark.parametrize('defect', [d for d in ref.DEFECTS if d != 'unstable_ties'])
def test_planted_defect_changes_a_golden_output(defect):
    changed = []
    for name in U.SETS:
        want = U.load_golden()[name][4]
        got = _restate(name, defect)
        changed += [(name, k) for k in RESULT_KEYS if not U.same_bits(got[k], want[k])]
    assert changed, 'the goldens do not notice the defect %r' % defect


def test_unstable_ties_defect_changes_the_tie_input():
    """the goldens have no equal scores (the reference does not define their order), so this defect is shown on the tie input"""
    gt, dt, K, I = U.tie_set()
    d = U.with_rows(dt)
    rows = d['rows']
    assert (rows[dt['category'] == 0, 4] == 0.123).sum() >= 8 and len(np.unique(rows[:, 4])) <= 10
    a, b = ref.run(gt, d, K), ref.run(gt, d, K, defect='unstable_ties')
    assert not U.same_bits(a['order'], b['order']) and not U.same_bits(a['prec'], b['prec'])


def test_convert_detections_equals_the_goldens_rows():
    from sniper_amd.evaluation import VOCBoxEvaluator
    for name in U.SETS:
        gt, dt, K, I, want = U.load_golden()[name]
        ev = VOCBoxEvaluator(gt, I, ['class%02d' % k for k in range(K)], True)
        rows, counts = ev.convert_detections(U.all_boxes_of(dt, K, I))
        assert rows.dtype == np.float64 and rows.tobytes() == want['rows'].tobytes(), name
        assert counts.shape == (K, I) and np.array_equal(counts.reshape(-1), np.bincount(dt['category'].astype(np.int64) * I + dt['image'], minlength=K * I))
    # float32 rows add their 1 in float32, float64 rows in float64, cell by cell; lists and empty cells pass
    gt, dt, K, I, want = U.load_golden()['edges']
    ev = VOCBoxEvaluator(gt, I, ['class%02d' % k for k in range(K)], True)
    boxes = U.all_boxes_of(dt, K, I)
    mixed = [[c.astype(np.float64) if (i + k) % 2 else c for i, c in enumerate(per)] for k, per in enumerate(boxes)]
    mixed[0] = [[] for _ in range(I)]
    rows2, _ = ev.convert_detections(mixed)
    slow = np.concatenate([U.result_rows(c) for per in mixed[1:] for c in per if len(c)])
    assert rows2.tobytes() == slow.tobytes() and rows2.tobytes() != want['rows'].tobytes()      # 0.35f + 1 differs between the two


def test_from_roidb_the_metric_rule_and_the_class_names():
    from sniper_amd import synthetic
    from sniper_amd.evaluation import VOC_CLASSES, VOCBoxEvaluator
    roidb = synthetic.make_roidb(n_images=6, seed=3, n_proposals=4, num_classes=21)
    n1 = len(roidb[1]['gt_classes'])
    roidb[1] = dict(roidb[1], gt_difficult=(np.arange(n1) % 2 == 0).astype(np.int32))
    ev = VOCBoxEvaluator.from_roidb(roidb, 21)
    assert ev.class_names == list(VOC_CLASSES) and len(VOC_CLASSES) == 20 and ev.use_07_metric and ev.thresholds == (0.5, 0.7)
    rows = [(i, int(c) - 1, b, n) for i, r in enumerate(roidb) for n, (b, c) in enumerate(zip(r['boxes'], r['gt_classes'])) if c > 0]
    assert len(rows) == len(ev.gt['image']) > 0 and any(c == 0 for r in roidb for c in r['gt_classes'])
    for j, (i, k, b, n) in enumerate(rows):
        assert ev.gt['image'][j] == i and ev.gt['category'][j] == k and list(ev.gt['bbox'][j]) == [float(v) + 1 for v in b]
        assert bool(ev.gt['difficult'][j]) == (i == 1 and n % 2 == 0)
    for year, want in (('2007', True), ('2009', True), ('2010', False), ('2012', False), ('SDS', True)):
        assert VOCBoxEvaluator.from_roidb(roidb, 21, year=year).use_07_metric is want
    named = VOCBoxEvaluator.from_roidb(roidb, 21, class_names=['__background__'] + ['c%d' % c for c in range(20)])
    assert named.class_names == ['c%d' % c for c in range(20)]
    assert VOCBoxEvaluator.from_roidb(synthetic.make_roidb(n_images=2, seed=3, n_proposals=4, num_classes=4), 4).class_names == ['class1', 'class2', 'class3']
    with pytest.raises(AssertionError):
        VOCBoxEvaluator.from_roidb(roidb, 21, class_names=['a', 'b'])


@pytest.mark.parametrize('use07', (True, False))
def test_summary_from_golden_arrays(use07):
    from sniper_amd.evaluation import VOCBoxResult
    for name in ('small', 'edges'):
        gt, dt, K, I, want = U.load_golden()[name]
        names = ['class%02d' % k for k in range(K)]
        res = VOCBoxResult(want['ap07'], want['ap_area'], np.zeros(K, np.int32), names, use07, U.THRESHOLDS)
        ap = want['ap07'] if use07 else want['ap_area']
        assert res.ap is ap and U.same_bits(res.mean_ap, np.array([np.mean(ap[0]), np.mean(ap[1])]))
        text = res.summary()
        assert text == ref.summary(ap, names, use07)
        lines = text.split('\n')
        assert len(lines) == 1 + 2 * (K + 1) + 1 and lines[0] == ('VOC07 metric? Y' if use07 else 'VOC07 metric? No')
        assert lines[1] == 'AP for class00 = %.4f' % ap[0, 0] and lines[K + 1] == 'Mean AP@0.5 = %.4f' % np.mean(ap[0])
        assert lines[K + 2] == '' and lines[-1] == 'Mean AP@0.7 = %.4f' % np.mean(ap[1]) and not text.endswith('\n')


def test_round_half_even_decimal_at_three_decimals():
    from sniper_amd.evaluation import round_half_even_decimal
    rs = np.random.RandomState(0)
    x = np.concatenate((rs.uniform(0, 1, 20000).astype(np.float32).astype(np.float64), np.arange(0, 2000) / 2000.0 + 0.00025,
                        np.arange(16) / 16.0 + 0.03125, [0.0005, 0.0015, 0.0025, 1.0, 0.0]))
    got = round_half_even_decimal(x, 3)
    assert got.tobytes() == np.array([float('{:.3f}'.format(v)) for v in x]).tobytes()
