"""CPU: the PASCAL VOC mask evaluation without a device.  tests/golden/vocsds_v1.npz holds what the reference's own voc_eval_sds
returned (tests/golden/make_vocsds_golden.py); the restatement tests/voc_sds_ref.py must equal it on the bits, each planted misreading
of the reference must move at least one of those numbers, and the host side of sniper_amd.evaluation (rounding, the instance pool, the
refusals, the summary) is checked against the restatement and plain Python."""
import numpy as np
import pytest

import voc_sds_ref as ref
import voc_sds_util as U


def _restate(name, defect=None):
    gt, dt, K, I, M, thr, ap = U.load_golden()[name]
    return ref.run(gt, dt, K, U.THRESHOLDS, thr, defect=defect)


@pytest.fixture(scope='module')
def restated():
    return {s: _restate(s) for s in U.SETS}


@pytest.mark.parametrize('name', U.SETS)
def test_restatement_equals_the_reference_on_the_bits(restated, name):
    ap = U.load_golden()[name][6]
    assert ap.dtype == np.float64 and ap.shape == restated[name]['ap07'].shape
    assert U.same_bits(restated[name]['ap07'], ap), (restated[name]['ap07'], ap)


def test_goldens_are_the_sets_of_the_generator_and_hold_what_the_issue_lists(restated):
    g = U.load_golden()
    for name, (gt, dt, K, I, M, thr) in U.make_sets().items():
        for k in U.GT_KEYS:
            assert g[name][0][k].tobytes() == gt[k].tobytes(), (name, k)
        for k in U.DT_KEYS:
            assert g[name][1][k].tobytes() == dt[k].tobytes(), (name, k)
        assert g[name][2:6] == (K, I, M, thr)
        for k in range(K):                                 # distinct scores: the reference's order is defined
            s = dt['raw'][dt['category'] == k, 4]
            assert len(np.unique(s)) == len(s), (name, k)
    gt, dt, K, I, M, thr, ap = g['seeded']
    assert (K, I, M, thr) == (3, 24, 28, 0.4) and 0.2 <= np.mean(ap[0]) <= 0.9
    w = restated['seeded']
    for k in range(K):
        c0, c1 = w['cls_off'][k], w['cls_off'][k + 1]
        assert all(w['dt_tp'][t, c0:c1].any() and w['dt_fp'][t, c0:c1].any() for t in range(2)), k
    assert ((w['iou'] > 0) & (w['iou'] < 1)).sum() > 20 and (w['dt_box'][:, :2] < 0).any()
    # the edge set (tests/voc_sds_util.py::edges_set), on the restatement's intermediate results
    gt, dt, K, I, M, thr, ap = g['edges']
    w = restated['edges']
    at = lambda i, k: np.flatnonzero((dt['image'] == i) & (dt['category'] == k))
    n = at(0, 0)[0]
    assert w['dt_iou'][n] == 0.5 and w['dt_tp'][0, n] == 1 and w['dt_fp'][1, n] == 1                       # exactly 0.5 is a match
    a, b = at(1, 0)
    assert w['dt_iou'][a] == 0.5 and w['dt_iou'][b] == 1.0 and w['dt_best'][a] == w['dt_best'][b] == 1     # the first of two equal overlaps
    assert (w['dt_tp'][0, a], w['dt_fp'][0, b], w['dt_fp'][1, a], w['dt_tp'][1, b]) == (1, 1, 1, 1)        # already_detect
    g1 = np.flatnonzero((gt['image'][w['gt_perm']] == 1) & (gt['category'][w['gt_perm']] == 0))
    assert w['gt_det'][0, g1].tolist() == [1, 0] and w['gt_det'][1, g1].tolist() == [2, 0]
    assert w['dt_best'][at(2, 0)[0]] == 0 and w['dt_iou'][at(2, 0)[0]] == -1000.0                          # no instance in the image
    z = at(3, 0)[0]
    assert w['dt_area'][z] == 0 and w['dt_iou'][z] == 0.0 and w['dt_best'][z] == 1                         # union < 1: overlap 0, a candidate
    assert w['npos'].tolist() == [4, 1, 2, 0, 1]
    c3 = slice(w['cls_off'][3], w['cls_off'][4])
    assert np.isnan(w['rec'][:, c3]).all() and w['rec'][:, c3].shape[1] == 2 and (ap[:, 3] == 0).all()     # detections, no instance anywhere
    assert w['cls_off'][5] == w['cls_off'][4] and (ap[:, 4] == 0).all()                                    # an instance, no detections
    box = w['dt_box'][at(4, 1)]
    wh = np.stack((box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1), axis=1).tolist()
    assert [1, 1] in wh and [12, 1] in wh and [1, 12] in wh and [2, 2] in wh and [0, 2, 4, 8] in box.tolist()
    assert (box[:, 0] < 0).any() and (box[:, 2] < 0).any()
    assert w['dt_area'][at(5, 2)[0]] == 16 and w['dt_area'][at(6, 2)[0]] == 0                              # on the threshold / a step below
    assert float(np.float32(thr)) < thr                      # why the edge set's threshold is 0.7: float32(0.7) < 0.7 < its successor


@pytest.mark.parametrize('defect', [d for d in ref.DEFECTS if d != 'unstable_ties'])
def test_planted_defect_changes_a_golden_number(defect):
    changed = [name for name in U.SETS if not U.same_bits(_restate(name, defect)['ap07'], U.load_golden()[name][6])]
    assert changed, 'the goldens do not notice the defect %r' % defect


def test_the_tie_rule_on_equal_scores_within_and_across_images():
    gt, dt, K, I, M, thr = U.tie_set()
    s = dt['raw'][dt['category'] == 0, 4]
    img = dt['image'][dt['category'] == 0]
    assert len(np.unique(s)) <= 8 < len(s)
    assert any(len(np.unique(img[s == v])) > 1 for v in np.unique(s)) and any((np.bincount(img[s == v]) > 1).any() for v in np.unique(s))
    a, b = ref.run(gt, dt, K, U.THRESHOLDS, thr), ref.run(gt, dt, K, U.THRESHOLDS, thr, defect='unstable_ties')
    assert not U.same_bits(a['order'], b['order']) and not U.same_bits(a['prec'], b['prec'])
    for k in range(K):                                     # arrival order inside every run of equal scores
        o = a['order'][a['cls_off'][k]:a['cls_off'][k + 1]]
        sc = dt['raw'][o, 4]
        assert (np.diff(sc) <= 0).all() and (np.diff(o)[np.diff(sc) == 0] > 0).all()


def test_host_rounding_and_its_refusal():
    from sniper_amd.evaluation import round_mask_boxes
    rows = np.array([[0.5, 1.5, 2.5, 3.5, 0.9], [-0.5, -1.5, -0.4, 7.49, 0.1], [-3.2, -2.7, 2.2, 3.0, 0.3]], np.float32)
    got = round_mask_boxes(rows)
    assert got.dtype == np.int32 and got.tolist() == [[0, 2, 2, 4], [0, -2, 0, 7], [-3, -3, 2, 3]]
    assert got.tolist() == [ref.round_box(r).tolist() for r in rows]
    with pytest.raises(ValueError, match=r'detection 1 has the box \[3, 0, 2, 5\] after rounding: x2 < x1 or y2 < y1'):
        round_mask_boxes(np.array([[0, 0, 1, 1, .5], [2.6, 0, 2.4, 5, .5]]))
    with pytest.raises(ValueError, match=r'detection 0 has the box \[0, 1, 4, 0\]'):
        round_mask_boxes(np.array([[0, 0.6, 4, 0.4, .5]]))
    with pytest.raises(ValueError, match='magnitude 2\\^30'):
        round_mask_boxes(np.array([[0, 0, 2.0 ** 30, 1, .5]]))
    assert round_mask_boxes(np.zeros((0, 5))).shape == (0, 4)


def test_evaluator_builds_the_instance_tables_and_refuses_what_it_must():
    from sniper_amd.evaluation import VOCSegmEvaluator
    gt, dt, K, I, M, thr, ap = U.load_golden()['edges']
    names = ['__background__'] + ['class%02d' % k for k in range(K)]
    ev = VOCSegmEvaluator(U.records_of(gt, I), I, names)
    assert ev.class_names == names[1:] and ev.thresholds == (0.5, 0.7) and ev.num_images == I
    assert np.array_equal(ev.gt['image'], np.sort(gt['image'])) and ev.gt['bound'].dtype == np.int32 and ev.gt['area'].dtype == np.int32
    o = np.argsort(gt['image'], kind='stable')              # records are per image: the instances arrive image-major
    assert np.array_equal(ev.gt['category'], gt['category'][o]) and np.array_equal(ev.gt['bound'], gt['bound'][o].astype(np.int32))
    assert ev.gt['area'].tolist() == [int(ref.gt_mask(gt, n).sum()) for n in o]
    bits, pix_off = ev._pool(np.arange(len(o))[::-1])
    assert bits.dtype == np.uint8 and pix_off.dtype == np.int64 and pix_off[-1] == len(bits) == len(gt['bits'])
    assert np.array_equal(bits[:pix_off[1]].reshape(ref.gt_mask(gt, o[-1]).shape), ref.gt_mask(gt, o[-1]))
    # bounds are rounded as the reference rounds them (halves to even) before the shape is compared
    VOCSegmEvaluator([[{'mask': np.ones((3, 3), bool), 'mask_bound': [0.5, 1.5, 1.5, 3.5], 'mask_cls': 1}]], 1, ['a'])
    with pytest.raises(ValueError, match=r'instance 0 of image 0 has a mask of shape \(2, 3\) in the bound \[0, 2, 2, 4\]'):
        VOCSegmEvaluator([[{'mask': np.ones((2, 3), bool), 'mask_bound': [0.5, 1.5, 1.5, 3.5], 'mask_cls': 1}]], 1, ['a'])
    with pytest.raises(ValueError, match='mask_cls 2, outside 1 .. 1'):
        VOCSegmEvaluator([[{'mask': np.ones((1, 1), bool), 'mask_bound': [0, 0, 0, 0], 'mask_cls': 2}]], 1, ['a'])
    with pytest.raises(ValueError, match='mask_cls 0'):
        VOCSegmEvaluator([[{'mask': np.ones((1, 1), bool), 'mask_bound': [0, 0, 0, 0], 'mask_cls': 0}]], 1, ['a'])
    with pytest.raises(AssertionError):
        VOCSegmEvaluator([[]], 2, ['a'])


def test_convert_detections_equals_the_restatements_rows_and_names_a_bad_box():
    from sniper_amd.evaluation import VOCSegmEvaluator
    for name in U.SETS:
        gt, dt, K, I, M, thr, ap = U.load_golden()[name]
        ev = VOCSegmEvaluator(U.records_of(gt, I), I, ['class%02d' % k for k in range(K)])
        all_boxes, all_masks = U.all_boxes_masks_of(dt, K, I, M)
        boxes, scores, masks, counts = ev.convert_detections(all_boxes, all_masks)
        assert boxes.dtype == np.int32 and scores.dtype == np.float64 and masks.dtype == np.float32
        assert np.array_equal(boxes, np.array([ref.round_box(r) for r in dt['raw']])) and masks.tobytes() == dt['masks'].tobytes()
        assert scores.tobytes() == dt['raw'][:, 4].astype(np.float64).tobytes()
        assert np.array_equal(counts.reshape(-1), np.bincount(dt['category'].astype(np.int64) * I + dt['image'], minlength=K * I))
    gt, dt, K, I, M, thr, ap = U.load_golden()['small']
    ev = VOCSegmEvaluator(U.records_of(gt, I), I, ['a', 'b'])
    all_boxes, all_masks = U.all_boxes_masks_of(dt, K, I, M)
    bad = [[c.copy() for c in per] for per in all_boxes]
    bad[2][2][0, :4] = [5.4, 5, 4.6, 7]                    # rounds to x1 = 5, x2 = 5: still a box
    ev.convert_detections(bad, all_masks)
    bad[2][2][0, :4] = [5.6, 5, 5.4, 7]                    # rounds to x1 = 6, x2 = 5
    with pytest.raises(ValueError, match=r'class 2, image 2: .*detection 0 has the box \[6, 5, 5, 7\] after rounding'):
        ev.convert_detections(bad, all_masks)
    short = [[m[:, :3] if len(m) else m for m in per] for per in all_masks]
    with pytest.raises(ValueError, match=r'all_masks\[1\]\[0\] has the shape \(2, 3, 4\) for 2 boxes'):
        ev.convert_detections(all_boxes, short)
    with pytest.raises(AssertionError):
        ev.convert_detections(all_boxes, all_masks[:-1])
    empty = ev.convert_detections([[[] for _ in range(I)] for _ in range(K + 1)], [[[] for _ in range(I)] for _ in range(K + 1)])
    assert empty[0].shape == (0, 4) and empty[3].sum() == 0


def test_evaluation_has_no_cpu_fallback(monkeypatch):
    import torch
    from sniper_amd.evaluation import evaluate_sds_voc
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    gt, dt, K, I, M, thr, ap = U.load_golden()['small']
    all_boxes, all_masks = U.all_boxes_masks_of(dt, K, I, M)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        evaluate_sds_voc(all_boxes, all_masks, U.records_of(gt, I), K + 1)


def test_summary_from_golden_arrays():
    from sniper_amd.evaluation import VOCSegmResult
    for name in U.SETS:
        gt, dt, K, I, M, thr, ap = U.load_golden()[name]
        names = ['class%02d' % k for k in range(K)]
        res = VOCSegmResult(ap, ap + 0.125, np.zeros(K, np.int32), names, U.THRESHOLDS)
        assert res.ap is ap and res.ap07 is ap and res.use_07_metric and U.same_bits(res.mean_ap, np.array([np.mean(ap[0]), np.mean(ap[1])]))
        text = res.summary()
        assert text == ref.summary(ap, names)
        lines = text.split('\n')
        assert len(lines) == 1 + 2 * (K + 1) + 1 and lines[1] == 'AP for class00 = %.4f' % ap[0, 0]
        assert lines[K + 1] == 'Mean AP@0.5 = %.4f' % np.mean(ap[0]) and lines[-1] == 'Mean AP@0.7 = %.4f' % np.mean(ap[1])
