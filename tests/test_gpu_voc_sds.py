"""-m gpu: sn_vocsds_mask_iou / sn_vocsds_match_iou / sn_voc_accumulate and sniper_amd.evaluation's VOC mask half against the
restatement tests/voc_sds_ref.py -- every byte of tp / fp and every bit of iou, rec, prec and ap07 -- and, for the golden sets, against
what the reference's voc_eval_sds returned (tests/golden/vocsds_v1.npz).  Every operand of the C-ABI runs sits between guard bytes
(tests/coco_eval_util.py::Guarded) and two runs must give identical bytes.  No tolerance appears except the derived bound of the
area AP (tests/voc_eval_util.py::assert_area_within_bound: 2 (n - 1) 2^-53 for n recall changes)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import voc_sds_ref as ref  # noqa: E402
import voc_sds_util as U  # noqa: E402


@pytest.mark.parametrize('name', U.SETS)
def test_device_equals_the_restatement_and_the_reference_goldens(name):
    gt, dt, K, I, M, thr, ap = U.load_golden()[name]
    got, want = U.check_device(gt, dt, K, U.THRESHOLDS, thr, name)
    assert U.same_bits(got['ap07'], ap), (got['ap07'], ap)
    assert got['dt_tp'].any() and got['dt_fp'].any()


SIZES_D = (0, 1, 63, 64, 65, 130)
SIZES_G = (0, 1, 2, 17)


def size_grid_set(seed, M=7):
    """one image per (D, G) pair in class 0 and again in class 2 (class 1 stays empty): exactly D detections and G instances in that
    problem.  Instances are small blobs on a coarse grid so that several detections claim one and equal overlaps occur; scores are
    quantised to 1 / 16 (ties within a problem)."""
    rng = np.random.RandomState(seed)
    pairs = [(d, g) for d in SIZES_D for g in SIZES_G]
    b = U.Builder(3, len(pairs), M, 0.4)
    for k in (0, 2):
        for i, (D, G) in enumerate(pairs):
            mine = []
            for _ in range(G):
                x, y, w, h = 8 * rng.randint(0, 5), 8 * rng.randint(0, 5), rng.randint(4, 12), rng.randint(4, 12)
                m = U._blob(rng, h, w)
                b.inst(i, k, x, y, m)
                canvas = np.zeros((64, 64), bool)
                canvas[y:y + h, x:x + w] = m
                mine.append(([x, y, x + w - 1, y + h - 1], canvas))
            for _ in range(D):
                if mine and rng.rand() < 0.8:
                    g, canvas = mine[rng.randint(len(mine))]
                    j = rng.randint(-2, 3, 4) * (rng.rand() < 0.6)
                    box = [g[0] + j[0], g[1] + j[1], g[2] + abs(j[2]), g[3] + abs(j[3])]
                    m = U.map_of(canvas, box, M, rng)
                else:
                    x, y = rng.uniform(-4, 40, 2)
                    box = [x, y, x + rng.uniform(1, 14), y + rng.uniform(1, 14)]
                    m = U.map_of(np.zeros((64, 64), bool), box, M, rng, noise=0.5)
                b.det(i, k, box, rng.randint(1, 17) / 16.0, m)
    return b.done()


def test_every_problem_size_with_an_empty_class_between():
    gt, dt, K, I, M, thr = size_grid_set(100)
    thresholds = tuple(np.linspace(0.2, 0.9, U.limits()[2]))            # SN_VOC_MAX_T thresholds
    got, want = U.check_device(gt, dt, K, thresholds, thr, 'sizes')
    D, G = np.diff(want['dt_off']), np.diff(want['gt_off'])
    assert sorted(set(zip(D.tolist(), G.tolist()))) == sorted((d, g) for d in SIZES_D for g in SIZES_G if d + g)
    assert want['cat_off'][1] == want['cat_off'][2] and (got['ap07'][:, 1] == 0).all() and got['npos'][1] == 0
    assert (got['dt_tp'].sum(axis=1) > 0).all() and (np.diff(got['dt_tp'].sum(axis=1).astype(int)) <= 0).all()
    assert ((got['iou'] > 0) & (got['iou'] < 1)).sum() > 100 and (got['ap07'][0, [0, 2]] > 0).all()


def test_box_widths_and_heights_around_the_workgroup_size():
    """a thread owns box columns c, c + T, ...: widths and heights of 1, T - 1, T, T + 1 and 2 T + 1, each with each, against two
    instances (one spans everything, one lies inside the last columns)"""
    T = U.limits()[4]
    sizes = [1, T - 1, T, T + 1, 2 * T + 1]
    rng = np.random.RandomState(5)
    b = U.Builder(1, 1, 14, 0.4)
    side = 2 * T + 9
    big = U._blob(np.random.RandomState(1), side, side)
    big[::7, :] = False
    b.inst(0, 0, -3, -2, big)
    b.inst(0, 0, T - 2, T - 3, np.ones((9, 11)))
    for n, (w, h) in enumerate((w, h) for w in sizes for h in sizes):
        m = (np.round(rng.uniform(0.1, 0.9, (14, 14)) * 32) / 32).astype(np.float32)
        b.det(0, 0, [0, 0, w - 1, h - 1], 1.0 - n / 64.0, m)
    gt, dt, K, I, M, thr = b.done()
    got, want = U.check_device(gt, dt, K, U.THRESHOLDS, thr, 'widths', twice=False)
    wh = np.stack((want['dt_box'][:, 2] + 1, want['dt_box'][:, 3] + 1), axis=1).tolist()
    assert wh == [[w, h] for w in sizes for h in sizes]
    assert (got['dt_area'] > 0).sum() >= 20 and got['dt_area'].max() > T * T and (got['iou'].reshape(-1, 2)[:, 0] > 0).sum() >= 20
    assert (got['iou'].reshape(-1, 2)[:, 1] > 0).sum() >= 9             # the boxes that reach the small instance


@pytest.mark.parametrize('M', (1, 14, 28))
def test_map_sizes(M):
    gt, dt, K, I, M_, thr = U.seeded_set(20 + M, 6, 2, M)
    got, want = U.check_device(gt, dt, K, U.THRESHOLDS, thr, 'M = %d' % M, twice=False)
    assert M_ == M and got['dt_tp'].any() and got['dt_fp'].any() and (got['dt_area'] > 0).any()


@pytest.mark.parametrize('thr', (0.4, 0.7))
def test_a_probability_on_the_threshold_and_one_float32_step_below(thr):
    """identity boxes (the box is M x M: every coefficient is 0): the map's own values are compared, >= in float32"""
    M = 14
    at = np.float32(thr)
    below, above = np.nextafter(at, np.float32(0)), np.nextafter(at, np.float32(1))
    b = U.Builder(1, 4, M, thr)
    half = np.zeros((M, M), np.float32)
    half[:, :7] = at
    half[:, 7:] = below
    for i, (m, score) in enumerate(((np.full((M, M), at), 0.9), (np.full((M, M), below), 0.8), (half, 0.7), (np.full((M, M), above), 0.6))):
        b.inst(i, 0, 3, 5, np.ones((M, M)))
        b.det(i, 0, [3, 5, 3 + M - 1, 5 + M - 1], score, m)
    gt, dt, K, I, M, thr = b.done()
    got, want = U.check_device(gt, dt, K, U.THRESHOLDS, thr, 'threshold %g' % thr, twice=False)
    assert got['dt_area'].tolist() == [M * M, 0, M * 7, M * M] and got['iou'].tolist() == [1.0, 0.0, 0.5, 1.0]
    assert got['dt_tp'][0].tolist() == [1, 0, 1, 1] and got['dt_tp'][1].tolist() == [1, 0, 0, 1]


def test_one_pixel_intersections_disjoint_identical_nested_and_negative_boxes():
    M = 4
    one = np.ones((M, M), np.float32)
    b = U.Builder(2, 2, M, 0.4)
    b.inst(0, 0, 4, 4, np.ones((4, 4)))                       # bound 4..7 x 4..7
    cases = [([1, 1, 4, 4], 'one pixel at the instance corner'), ([7, 7, 10, 10], 'one pixel at the opposite corner'),
             ([7, 0, 9, 4], 'one pixel, top right'), ([0, 7, 4, 12], 'one pixel, bottom left'), ([0, 0, 3, 3], 'disjoint, touching'),
             ([20, 20, 23, 23], 'disjoint, far'), ([4, 4, 7, 7], 'identical'), ([5, 5, 6, 6], 'nested inside (exact 2x)'),
             ([2, 2, 9, 9], 'the instance nested inside'), ([-6, -6, -2, -2], 'wholly negative'), ([-3, -3, 5, 5], 'partly negative')]
    for n, (box, _) in enumerate(cases):
        b.det(0, 0, box, 1.0 - n / 32.0, one)
    # class 1: an instance at negative coordinates (nothing here knows an image) met by boxes on both sides of the origin
    b.inst(1, 1, -5, -4, np.tri(6, 7))
    b.det(1, 1, [-5, -4, 1, 1], 0.9, one)
    b.det(1, 1, [-2.5, -1.5, 3.5, 2.5], 0.8, np.tri(M, M, dtype=np.float32))
    b.det(1, 1, [-5, 1, -5, 1], 0.7, one)
    gt, dt, K, I, M, thr = b.done()
    got, want = U.check_device(gt, dt, K, U.THRESHOLDS, thr, 'geometry')
    ov = got['iou'][:len(cases)]
    assert ov[:4].tolist() == [1 / 31.0, 1 / 31.0, 1 / 30.0, 1 / 45.0] and ov[4:6].tolist() == [0.0, 0.0] and ov[6] == 1.0 and ov[7] == 4 / 16.0 and ov[8] == 16 / 64.0
    assert ov[9] == 0.0 and ov[10] == 4 / (81 + 16 - 4.0) and got['dt_area'][:len(cases)].tolist() == [16, 16, 15, 30, 16, 16, 16, 4, 64, 25, 81]
    assert got['iou'][len(cases)] == 0.5 and 0 < got['iou'][len(cases) + 1] < 1 and got['iou'][len(cases) + 2] == 1 / 21.0


def test_problems_over_the_caps_are_refused_before_any_launch():
    import torch
    from sniper_amd._lib import SniperHipError
    from sniper_amd.evaluation import VOCSegmEvaluator
    max_dt, max_gt, max_t, max_m = U.limits()[:4]
    rec = lambda n: [[{'mask': np.ones((2, 2), bool), 'mask_bound': [0, 0, 1, 1], 'mask_cls': 1} for _ in range(n)]]
    dets = lambda n, M: ([[[]], [np.tile(np.array([[0, 0, 3, 3, 0.5]], np.float32), (n, 1))]], [[[]], [np.ones((n, M, M), np.float32)]])
    torch.cuda.synchronize()
    for records, (boxes, masks), thresholds, words in (
            (rec(1), dets(max_dt + 1, 2), (0.5,), ('sn_vocsds_match_iou', 'a problem has %d detections' % (max_dt + 1))),
            (rec(max_gt + 1), dets(1, 2), (0.5,), ('sn_vocsds_mask_iou', 'a problem has %d instances' % (max_gt + 1))),
            (rec(1), dets(1, max_m + 1), (0.5,), ('sn_vocsds_mask_iou', '1 <= M <= %d' % max_m)),
            (rec(1), dets(1, 2), tuple(np.linspace(0.1, 0.9, max_t + 1)), ('sn_vocsds_match_iou', '1 <= T <= %d' % max_t))):
        with pytest.raises(SniperHipError) as e:
            VOCSegmEvaluator(records, 1, ['a'], thresholds).evaluate(boxes, masks)
        assert all(w in str(e.value) for w in words), str(e.value)
    ok = VOCSegmEvaluator(rec(max_gt), 1, ['a']).evaluate(*dets(max_dt, 2))          # at the caps: accepted
    assert ok.npos.tolist() == [max_gt] and ok.timing['pairs'] == max_dt * max_gt
    torch.cuda.synchronize()


def test_evaluator_and_the_one_call_form_on_the_goldens(capsys):
    """the public interface: records, all_boxes and all_masks -> rounding, pools, offsets -> three entry points -> the summary"""
    from sniper_amd.evaluation import VOCSegmEvaluator, evaluate_sds_voc
    for name in U.SETS:
        gt, dt, K, I, M, thr, ap = U.load_golden()[name]
        names = ['class%02d' % k for k in range(K)]
        all_boxes, all_masks = U.all_boxes_masks_of(dt, K, I, M)
        records = U.records_of(gt, I)
        res = VOCSegmEvaluator(records, I, ['__background__'] + names).evaluate(all_boxes, all_masks, binary_thresh=thr, return_matches=True)
        # the records arrive image-major, the restatement's instances in the set's own order: compare on the evaluator's order
        o = np.argsort(gt['image'], kind='stable')
        gt2 = dict({k: gt[k][o] for k in ('image', 'category', 'bound')}, bits=np.concatenate([gt['bits'][gt['pix_off'][n]:gt['pix_off'][n + 1]] for n in o]),
                   pix_off=np.concatenate([[0], np.cumsum(np.diff(gt['pix_off'])[o])]))
        want = ref.run(gt2, dt, K, U.THRESHOLDS, thr)
        assert U.same_bits(res.ap07, ap) and U.same_bits(res.ap07, want['ap07']) and np.array_equal(res.npos, want['npos']) and res.ap is res.ap07
        U.assert_same_bits(res.matches, want, keys=('dt_box', 'dt_area', 'iou', 'iou_off', 'dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det', 'order', 'rec', 'prec'),
                           what='evaluator ' + name)
        U.assert_area_within_bound(res.ap_area, want['ap_area'], U.recall_changes(want['rec'], want['cls_off']), 'evaluator ' + name)
        assert res.summary() == ref.summary(ap, names) and len(res.summary().split('\n')) == 2 * (K + 1) + 2
        assert set(res.timing) == {'host_s', 'upload_s', 'kernels_s', 'mask_iou_s', 'match_s', 'accumulate_s', 'download_s', 'problems',
                                   'detections', 'instances', 'pairs'}
        one = evaluate_sds_voc(all_boxes, all_masks, records, K + 1, class_names=names, binary_thresh=thr)
        assert U.same_bits(one.ap07, ap) and one.class_names == names
        print(name)
        print(one.summary())
    assert 'Mean AP@0.5 = ' in capsys.readouterr().out
    gt, dt, K, I, M, thr, ap = U.load_golden()['small']
    all_boxes, all_masks = U.all_boxes_masks_of(dt, K, I, M)
    nothing = VOCSegmEvaluator([[] for _ in range(I)], I, ['a', 'b'])
    empty_b, empty_m = [[[] for _ in range(I)] for _ in range(K + 1)], [[[] for _ in range(I)] for _ in range(K + 1)]
    r = nothing.evaluate(empty_b, empty_m)
    assert (r.ap == 0).all() and (r.npos == 0).all()
    r = nothing.evaluate(all_boxes, all_masks)                         # detections, no instance anywhere: rec = nan, AP 0
    assert (r.ap07 == 0).all() and np.isnan(r.ap_area).all() and (r.npos == 0).all()
    r = VOCSegmEvaluator(U.records_of(gt, I), I, ['a', 'b']).evaluate(empty_b, empty_m)      # instances, no detections
    assert (r.ap == 0).all() and r.npos.tolist() == [2, 3]


def test_overlap_equals_sn_rle_iou_of_the_pasted_detection_wherever_the_box_gate_passes():
    """boxes inside an image: the detection pasted by sn_rle_paste and the instance encoded in the same image give, through
    sn_rle_iou, the overlap of sn_vocsds_mask_iou on the bits -- unless the bounding boxes of the two encoded masks do not meet, where
    sn_rle_iou answers 0 by its gate"""
    import coco_segm_ref as cref
    import coco_segm_util as CU
    from sniper_amd.evaluation import rle_paste
    gt, dt, K, I, M, thr, ap = U.load_golden()['seeded']
    want = ref.run(gt, dt, K, U.THRESHOLDS, thr)
    inside = (want['dt_box'][:, 0] >= 0) & (want['dt_box'][:, 1] >= 0)
    keep = np.flatnonzero(inside)
    assert 40 < len(keep) < len(inside)
    dt2 = {k: dt[k][keep] for k in U.DT_KEYS}
    want = ref.run(gt, dt2, K, U.THRESHOLDS, thr)
    got = U.device_run(gt, dt2, K, U.THRESHOLDS, thr, want)
    assert U.same_bits(got['iou'], want['iou'])
    bound = np.round(gt['bound']).astype(int)
    hw = np.zeros((I, 2), np.int32)                                      # an image that holds everything of its index
    for i in range(I):
        ys = np.concatenate((bound[gt['image'] == i, 3], want['dt_box'][dt2['image'] == i, 3]))
        xs = np.concatenate((bound[gt['image'] == i, 2], want['dt_box'][dt2['image'] == i, 2]))
        hw[i] = ys.max() + 1, xs.max() + 1
    g_rle = []
    for n in range(len(gt['image'])):
        img = np.zeros(hw[gt['image'][n]], np.uint8)
        img[bound[n, 1]:bound[n, 3] + 1, bound[n, 0]:bound[n, 2] + 1] = ref.gt_mask(gt, n)
        g_rle.append(cref.rle_encode(img))
    d_rle = rle_paste(dt2['masks'], want['dt_box'], hw[dt2['image']], thr)
    zeros = np.zeros(len(g_rle), np.int32)
    ev = dict(want, dt_perm=np.arange(len(keep)))
    rle_iou, iou_off, d_rows, g_rows = CU.device_iou(ev, {'rle': g_rle, 'hw': hw[gt['image']], 'iscrowd': zeros, 'ignore': zeros},
                                                     {'rle': d_rle, 'hw': hw[dt2['image']], 'score': dt2['raw'][:, 4]})
    assert np.array_equal(iou_off, want['iou_off']) and np.array_equal(d_rows[:, 5], got['dt_area'])
    gate = np.zeros(len(rle_iou), bool)
    for p in range(len(want['dt_off']) - 1):
        for d in range(want['dt_off'][p], want['dt_off'][p + 1]):
            for j, g in enumerate(range(want['gt_off'][p], want['gt_off'][p + 1])):
                a, b = d_rows[d, :4], g_rows[g, :4]
                w = min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0])
                h = min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1])
                gate[iou_off[p] + (d - want['dt_off'][p]) * (want['gt_off'][p + 1] - want['gt_off'][p]) + j] = w > 0 and h > 0
    assert gate.sum() > 30 and (~gate).sum() > 5
    assert U.same_bits(rle_iou[gate], got['iou'][gate]) and (rle_iou[~gate] == 0).all() and (got['iou'][gate] > 0).sum() > 20


def test_instances_submitted_as_detections_score_one():
    """the closed loop: rectangular instances, detections equal to their bounds with constant-1 maps"""
    rng = np.random.RandomState(3)
    K, I, M = 3, 12, 14
    b = U.Builder(K, I, M, 0.4)
    n = 0
    for i in range(I):
        for j in range(rng.randint(1, 4)):
            w, h = rng.randint(1, 40, 2)
            x, y = 50 * j + rng.randint(-5, 5), rng.randint(-5, 30)          # disjoint in x: every detection meets its own instance only
            k = int(rng.randint(K))
            b.inst(i, k, x, y, np.ones((h, w)))
            b.det(i, k, [x, y, x + w - 1, y + h - 1], 1.0 - n / 128.0, np.ones((M, M), np.float32))
            n += 1
    gt, dt, K, I, M, thr = b.done()
    got, want = U.check_device(gt, dt, K, U.THRESHOLDS, thr, 'closed loop')
    assert got['dt_tp'].all() and not got['dt_fp'].any() and (got['dt_iou'] == 1.0).all() and (got['prec'] == 1.0).all()
    assert np.array_equal(got['dt_area'], (want['dt_box'][:, 2] - want['dt_box'][:, 0] + 1) * (want['dt_box'][:, 3] - want['dt_box'][:, 1] + 1))
    assert U.same_bits(got['ap07'], want['ap07']) and (got['ap07'] > 0.999).all() and (got['rec'][:, want['cls_off'][1:] - 1] == 1.0).all()
