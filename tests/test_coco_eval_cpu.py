"""CPU: the COCO box evaluation without a device.  tests/golden/cocoeval_v1.npz was written by the reference's own cocoeval.py and
bbIou (tests/golden/make_cocoeval_golden.py); the restatement tests/coco_eval_ref.py must equal every array in it on the bits, each
of five planted misreadings of the reference must change at least one of them, and the host side of sniper_amd.evaluation (ground
truth from a roidb, the reference's rounding of the result rows, the CSR offsets of the problems) is checked against plain Python."""
import numpy as np
import pytest

import coco_eval_ref as ref
import coco_eval_util as U

DEFECTS = ('first_of_equal', 'gt_threshold', 'exclusive_area', 'unstable_ties', 'no_crowd_rematch')


@pytest.fixture(scope='module')
def restated():
    return {s: ref.run(gt, dt, K) for s, (gt, dt, K, I, _) in U.load_golden().items()}


@pytest.mark.parametrize('name', U.SETS)
def test_restatement_equals_the_reference_on_the_bits(restated, name):
    want = U.load_golden()[name][4]
    U.assert_same_bits(restated[name], want, keys=U.RESULT_KEYS, what=name)


def test_goldens_hold_what_the_issue_lists():
    g = U.load_golden()
    assert g['small'][2:4] == (5, 40) and g['large'][2:4] == (80, 300) and 2000 <= len(g['large'][1]['score']) <= 4000
    for name in ('small', 'large'):
        res = g[name][4]
        assert 0.2 <= res['stats'][0] <= 0.8 and np.mean(res['precision'] > -1) >= 0.9
    for name in U.SETS:
        matched = g[name][4]['dt_match'][0] != 0
        assert matched.any(axis=1).all() and (~matched).any(axis=1).all()
    gt, dt, K, I, res = g['hand']
    assert (res['precision'][:, :, 4] == -1).all() and (res['precision'][:, :, 5] == -1).all()       # absent; every box ignored
    counts = np.bincount(dt['category'].astype(np.int64) * I + dt['image'], minlength=K * I)
    assert counts.max() == 130


@pytest.mark.parametrize('defect', DEFECTS)
def test_planted_defect_changes_a_golden_output(defect):
    changed = []
    for name, (gt, dt, K, I, want) in U.load_golden().items():
        if name == 'large':
            continue                                  # the two small sets decide; the large one only costs time
        got = ref.run(gt, dt, K, defect=defect)
        changed += [(name, k) for k in U.RESULT_KEYS if got[k].tobytes() != want[k].tobytes()]
    assert changed, 'the goldens do not notice the defect %r' % defect


def test_round_half_even_decimal_is_the_builtin_round():
    from sniper_amd.evaluation import round_half_even_decimal
    rs = np.random.RandomState(0)
    x = np.concatenate((rs.uniform(-50, 700, 20000).astype(np.float32).astype(np.float64), rs.uniform(0, 1, 20000),
                        np.arange(-40, 40) / 8.0, np.arange(0, 2000) / 20.0 + 0.05, [0.25, 0.35, 2.675, 1e-9, -0.05, 0.15, 1e17, 0.0]))
    for nd in (1, 8):
        got = round_half_even_decimal(x, nd)
        want = np.array([round(float(v), nd) for v in x])
        assert got.tobytes() == want.tobytes()
    assert (np.round(x, 1) != round_half_even_decimal(x, 1)).any()          # np.round is not the builtin: that is why this exists


def _roidb_and_boxes(n_images=20, num_classes=11):
    from sniper_amd import synthetic
    roidb = synthetic.make_roidb(n_images=n_images, seed=3, n_proposals=4, num_classes=num_classes)
    return roidb, num_classes


def test_from_roidb_and_detection_conversion():
    from sniper_amd.evaluation import COCOBoxEvaluator
    roidb, nc = _roidb_and_boxes()
    roidb[1] = dict(roidb[1], gt_iscrowd=(np.arange(len(roidb[1]['gt_classes'])) % 3 == 0).astype(np.int32),
                    gt_areas=np.arange(len(roidb[1]['gt_classes']), dtype=np.float64) + 0.5)
    ev = COCOBoxEvaluator.from_roidb(roidb, nc)
    assert ev.image_ids == list(range(1, len(roidb) + 1)) and ev.cat_ids == list(range(1, nc))
    rows = [(i, int(c) - 1, b, n) for i, r in enumerate(roidb) for n, (b, c) in enumerate(zip(r['boxes'], r['gt_classes'])) if c > 0]
    assert len(rows) == len(ev.gt['image']) > 0 and any(c == 0 for r in roidb for c in r['gt_classes'])
    for j, (i, k, b, n) in enumerate(rows):
        b = [float(v) for v in b]
        xywh = [b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1]
        assert ev.gt['image'][j] == i and ev.gt['category'][j] == k and list(ev.gt['bbox'][j]) == xywh
        assert ev.gt['area'][j] == (n + 0.5 if i == 1 else xywh[2] * xywh[3])
        assert bool(ev.gt['iscrowd'][j]) == (i == 1 and n % 3 == 0) and not ev.gt['ignore'][j]
    # detections: float32 rows with awkward decimals -> the reference's result rows (coco.py:36-48, loadRes)
    rs = np.random.RandomState(1)
    all_boxes = [[[] for _ in roidb]] + [[None] * len(roidb) for _ in range(nc - 1)]
    want = []
    for c in range(1, nc):
        for i in range(len(roidb)):
            n = rs.randint(0, 4)
            xy = rs.uniform(0, 300, (n, 2))
            d = np.hstack((xy, xy + rs.uniform(1, 200, (n, 2)), rs.uniform(0, 1, (n, 1)))).astype(np.float32)
            d[:, :4] = np.round(d[:, :4] * 20) / 20                    # many x.x5 values: the halves
            all_boxes[c][i] = d
            for row in d.astype(float):
                w, h = row[2] - row[0] + 1, row[3] - row[1] + 1
                bb = [round(float(row[0]), 1), round(float(row[1]), 1), round(float(w), 1), round(float(h), 1)]
                want.append(bb + [round(float(row[4]), 8), bb[2] * bb[3]])
    got, counts = ev.convert_detections(all_boxes)
    assert got.tobytes() == np.array(want, np.float64).tobytes()
    assert counts.shape == (nc - 1, len(roidb)) and counts.sum() == len(want)
    assert counts[2, 5] == len(all_boxes[3][5])


def test_problem_offsets_equal_the_restatement():
    from sniper_amd.evaluation import COCOBoxEvaluator
    for name in ('small', 'hand'):
        gt, dt, K, I, _ = U.load_golden()[name]
        ev = COCOBoxEvaluator(gt, range(1, I + 1), range(1, K + 1))
        counts = np.bincount(dt['category'].astype(np.int64) * I + dt['image'], minlength=K * I).reshape(K, I)
        pr = ev._problems(counts, 100)
        want = ref.evaluate(gt, dt, K)
        for k in ('dt_off', 'gt_off', 'kp_off', 'cat_off'):
            assert pr[k].dtype == np.int32 and np.array_equal(pr[k], want[k]), (name, k)
        assert np.array_equal(pr['gt_order'], want['gt_perm']) and pr['P'] == len(want['prob_cat'])
        assert pr['max_dt'] == np.diff(want['dt_off']).max() and pr['max_gt'] == np.diff(want['gt_off']).max()


def test_ground_truth_as_detections_scores_one():
    """every box submitted as a detection of score 1: AR@100 = 1 exactly; AP is the mean of tp / (tp + 0 + eps), each within one
    rounding of 1 / (1 + 2.2e-16), so 1 - 1e-15 < AP <= 1"""
    from sniper_amd.evaluation import COCOBoxEvaluator
    roidb, nc = _roidb_and_boxes()
    ev = COCOBoxEvaluator.from_roidb(roidb, nc)
    n = len(ev.gt['image'])
    gt = dict(ev.gt, iscrowd=ev.gt['iscrowd'].astype(np.int32), ignore=ev.gt['ignore'].astype(np.int32))
    dt = {'image': gt['image'], 'category': gt['category'], 'bbox': gt['bbox'], 'score': np.ones(n), 'area': gt['area']}
    out = ref.run(gt, dt, nc - 1)
    assert 1 - 1e-15 < out['stats'][0] <= 1 and out['stats'][8] == 1.0
    assert 1 - 1e-15 < out['stats'][1] <= 1 and 1 - 1e-15 < out['stats'][2] <= 1


def test_unsupported_modes_say_so():
    from sniper_amd.evaluation import COCOBoxEvaluator, Params
    gt = U.load_golden()['hand'][0]
    p = Params()
    p.useSegm = 1
    with pytest.raises(NotImplementedError, match='useSegm'):
        COCOBoxEvaluator(gt, range(12), range(6), p)
    p = Params()
    p.useCats = 0
    with pytest.raises(NotImplementedError, match='useCats'):
        COCOBoxEvaluator(gt, range(12), range(6), p)
    d = Params()
    r = ref.Params()
    assert d.iouThrs.tobytes() == r.iouThrs.tobytes() and d.recThrs.tobytes() == r.recThrs.tobytes()
    assert d.maxDets == [1, 10, 100] and d.areaRng == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_summary_lines_and_stats_from_golden_arrays():
    from sniper_amd.evaluation import COCOBoxResult, Params
    for name in ('small', 'hand'):
        res = U.load_golden()[name][4]
        out = COCOBoxResult(res['precision'], res['recall'], Params(), range(res['precision'].shape[2]))
        assert out.stats.tobytes() == res['stats'].tobytes()
        lines = out.summary().split('\n')
        assert len(lines) == 12
        assert lines[0] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = %.3f' % res['stats'][0]
        assert lines[6] == ' Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = %.3f' % res['stats'][6]
        pr = res['precision'][:, :, :, 0, 2]
        for k in range(pr.shape[2]):
            sel = pr[:, :, k][pr[:, :, k] > -1]
            assert (np.isnan(out.per_class_ap[k]) and sel.size == 0) or out.per_class_ap[k] == np.mean(sel)
