"""CPU: the restatement of the reference's mask evaluation (tests/coco_segm_ref.py) equals tests/golden/cocosegm_v1.npz -- written
from the reference's own maskApi.c and cocoeval.py -- on the bits, for all three sets and every stage; the host helpers of
sniper_amd.evaluation (string counts, pools, chunks, the order of the detections) and its ValueErrors."""
import numpy as np
import pytest

import coco_segm_ref as ref
import coco_segm_util as U
from coco_eval_util import assert_same_bits


@pytest.fixture(scope='module')
def golden():
    return U.load_golden()


@pytest.fixture(scope='module')
def runs(golden):
    """the restatement's results, computed once"""
    out = {}
    for s in U.SETS:
        gt, dt = U.ref_inputs(golden[s])
        out[s] = ref.run(gt, dt, golden[s]['K'])
    return out


@pytest.mark.parametrize('s', U.SETS)
def test_polygons_and_bitmaps_encode_to_the_reference_counts(golden, s):
    d, made = golden[s], U.make_sets()[s]
    assert len(made['gt']) == len(d['gt_counts']) and len(made['dt']) == len(d['dt_counts'])
    polys = 0
    for n, a in enumerate(made['gt']):
        h, w = (int(v) for v in d['sizes'][a['image']])
        if a['seg'][0] == 'poly':
            assert int(d['gt_form'][n]) == U.FORM_POLY
            got = ref.rle_from_polys(d['gt_polys'][n], h, w)
            polys += 1
        else:
            got = ref.rle_encode(a['seg'][1])
        assert np.array_equal(got, d['gt_counts'][n]), (s, n, a.get('case'), got, d['gt_counts'][n])
    for n, a in enumerate(made['dt']):
        if a['mask'] is not None:
            assert np.array_equal(ref.rle_encode(a['mask']), d['dt_counts'][n]), (s, n)
    assert polys > 0 or s != 'edge'


@pytest.mark.parametrize('s', U.SETS)
def test_string_counts_decode_to_the_reference_counts(golden, s):
    from sniper_amd.evaluation import rle_from_string
    d = golden[s]
    strings = [n for n in range(len(d['gt_form'])) if int(d['gt_form'][n]) == U.FORM_STRING]
    assert strings or s == 'hand'
    for n in strings:
        assert np.array_equal(ref.rle_from_string(d['gt_strings'][n]), d['gt_counts'][n])
        got = rle_from_string(d['gt_strings'][n])
        assert got.dtype == np.uint32 and np.array_equal(got, d['gt_counts'][n])


def test_string_counts_with_negative_differences():
    """counts that fall by more than 15 need the sign bit and several characters; the pairs below were written out by hand from
    rleToString's rule: [3, 1, 1, 40, 1] -> differences 3, 1, -2, 39, 0"""
    from sniper_amd.evaluation import rle_from_string
    enc = lambda x: ''.join(chr(48 + c) for c in _leb(x))
    text = enc(3) + enc(1) + enc(1) + enc(40 - 1) + enc(1 - 1)
    assert np.array_equal(rle_from_string(text), [3, 1, 1, 40, 1]) and np.array_equal(ref.rle_from_string(text), [3, 1, 1, 40, 1])
    text = enc(100) + enc(2) + enc(3) + enc(1000) + enc(7 - 3)
    assert np.array_equal(rle_from_string(text), [100, 2, 3, 1002, 7])
    text = enc(50) + enc(2) + enc(60) + enc(1 - 2) + enc(5 - 60)
    assert np.array_equal(rle_from_string(text), [50, 2, 60, 1, 5])
    with pytest.raises(ValueError, match='ends inside a count'):
        rle_from_string(chr(48 + 0x20))


def _leb(x):
    """rleToString's characters for one (possibly negative) difference: 5 bits each, 0x20 = more"""
    out = []
    more = True
    while more:
        c = x & 0x1f
        x >>= 5
        more = (x != -1) if (c & 0x10) else (x != 0)
        out.append(c | (0x20 if more else 0))
    return out


@pytest.mark.parametrize('s', U.SETS)
def test_area_and_bbox_rows(golden, s):
    d = golden[s]
    rows = ref.stats_rows(d['dt_counts'], d['sizes'][d['dt_image']], d['dt_score'])
    assert rows[:, :4].tobytes() == d['dt_bbox'].tobytes() and rows[:, 5].tobytes() == d['dt_area'].tobytes()
    assert rows[:, 4].tobytes() == d['dt_score'].tobytes()


@pytest.mark.parametrize('s', U.SETS)
def test_iou_matrices(golden, runs, s):
    d, r = golden[s], runs[s]
    assert np.array_equal(r['iou_off'], d['iou_off'])
    assert r['iou'].tobytes() == d['iou'].tobytes()


def test_the_column_wrap_pair_scores_zero():
    g, d = np.array(U.QUIRK_GT, np.uint32), np.array(U.QUIRK_DT, np.uint32)
    common = int((U.from_counts(g, 10, 10) & U.from_counts(d, 10, 10)).sum())
    assert common == 2 and ref.rle_iou(d, g, (10, 10), 0) == 0.0
    assert ref.rle_to_bbox(g, 10, 10) == [3.0, 2.0, 2.0, 4.0] and ref.rle_to_bbox(d, 10, 10) == [4.0, 0.0, 1.0, 2.0]


@pytest.mark.parametrize('s', U.SETS)
def test_matches_and_curves(golden, runs, s):
    d, r = golden[s], runs[s]
    assert_same_bits(r, d['res'], keys=('dt_rank', 'dt_scores', 'dt_match', 'dt_ignore', 'gt_match', 'gt_ignore', 'precision', 'recall', 'stats'),
                     what=s)


# ---- the host side of sniper_amd.evaluation ---------------------------------------------------------
def _evaluator(d, **kw):
    from sniper_amd.evaluation import COCOSegmEvaluator
    return COCOSegmEvaluator(U.gt_dict(d, polygons=False), range(1, d['I'] + 1), range(1, d['K'] + 1), d['sizes'], **kw)


@pytest.mark.parametrize('s', U.SETS)
def test_evaluator_decodes_the_ground_truth(golden, s):
    d = golden[s]
    ev = _evaluator(d)
    assert len(ev.gt_rle) == len(d['gt_counts'])
    for got, want in zip(ev.gt_rle, d['gt_counts']):
        assert got.dtype == np.uint32 and np.array_equal(got, want)


def test_detections_come_in_class_major_order_with_unrounded_scores(golden):
    d = golden['seeded']
    ev = _evaluator(d)
    boxes, masks = U.detections_of(d)
    boxes[1][0] = np.concatenate((boxes[1][0], [[0, 0, 0, 0, 0.123456789012345]]))
    masks[1][0] = list(masks[1][0]) + [{'size': [int(v) for v in d['sizes'][0]], 'counts': [int(np.prod(d['sizes'][0]))]}]
    scores, rles, counts = ev.convert_detections(boxes, masks)
    order = np.lexsort((np.arange(len(d['dt_image'])), d['dt_image'], d['dt_category']))
    n0 = int(counts[0, 0]) - 1                        # the added detection is the last row of cell (class 1, image 0)
    assert scores[n0] == 0.123456789012345
    assert np.array_equal(np.delete(scores, n0), d['dt_score'][order])
    kept = rles[:n0] + rles[n0 + 1:]
    assert all(np.array_equal(a, d['dt_counts'][n]) for a, n in zip(kept, order))
    assert counts.sum() == len(order) + 1


def test_chunks_cover_the_problems_in_order(golden):
    ev = _evaluator(golden['hand'], chunk_elements=10)
    cost = np.array([3, 4, 5, 30, 1, 1, 9, 0, 0, 2])
    chunks = ev._chunks(cost)
    assert chunks[0][0] == 0 and chunks[-1][1] == len(cost) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert all(cost[a:b].sum() <= 10 or b - a == 1 for a, b in chunks) and (3, 4) in chunks
    assert ev._chunks(np.zeros(0, np.int64)) == []
    assert _evaluator(golden['hand'], chunk_elements=1 << 30)._chunks(cost) == [(0, len(cost))]


def test_value_errors(golden):
    from sniper_amd.evaluation import COCOBoxEvaluator, COCOSegmEvaluator, Params, rle_counts
    d = golden['hand']
    gt = U.gt_dict(d)
    args = (range(1, d['I'] + 1), range(1, d['K'] + 1), d['sizes'])
    bad = dict(gt, segmentation=list(gt['segmentation']))
    bad['segmentation'][2] = {'size': [5, 5], 'counts': [25]}
    with pytest.raises(ValueError, match='annotation 2: the mask is 5 x 5, its image 8 x 8'):
        COCOSegmEvaluator(bad, *args)
    bad['segmentation'][2] = {'size': [8, 8], 'counts': [10, 5, 48]}
    with pytest.raises(ValueError, match='annotation 2: the counts sum to 63'):
        COCOSegmEvaluator(bad, *args)
    bad['segmentation'][2] = {'size': [8, 8], 'counts': [10, 0, 54]}
    with pytest.raises(ValueError, match='annotation 2: an empty run'):
        COCOSegmEvaluator(bad, *args)
    for poly, words in (([], 'non-empty list'), ([[0, 0, 4]], 'x0, y0, x1, y1'), ([[0, 0, float('nan'), 1]], 'finite'), ([[]], 'at least one vertex')):
        bad['segmentation'][2] = poly          # a malformed polygon annotation is refused on the host, before a device is asked for
        with pytest.raises(ValueError, match='annotation 2: .*' + words):
            COCOSegmEvaluator(bad, *args)
    with pytest.raises(ValueError, match='h \\* w < 2\\^31'):
        COCOSegmEvaluator(gt, args[0], args[1], np.full((d['I'], 2), 1 << 16))
    assert np.array_equal(rle_counts({'size': [2, 3], 'counts': [0, 6]}, 2, 3, 'x'), [0, 6])          # a leading 0 is the all-one mask
    ev = COCOSegmEvaluator(gt, *args)
    boxes, masks = U.detections_of(d)
    masks[1][0] = masks[1][0][:1]
    with pytest.raises(ValueError, match=r'all_masks\[1\]\[0\] has 1 masks, all_boxes\[1\]\[0\] 2 rows'):
        ev.convert_detections(boxes, masks)
    boxes, masks = U.detections_of(d)
    masks[1][0] = [masks[1][0][0], {'size': [6, 6], 'counts': [35]}]
    with pytest.raises(ValueError, match=r'detection 1 of all_masks\[1\]\[0\]: the counts sum to 35'):
        ev.convert_detections(boxes, masks)
    masks[1][0] = np.zeros((2, 28, 27), np.float32)
    with pytest.raises(ValueError, match=r'all_masks\[1\]\[0\] is neither a list of RLE dicts nor \(n, M, M\) probabilities'):
        ev.convert_detections(boxes, masks)
    masks[1][0] = np.zeros((2, 28, 28), np.float32)
    boxes[1][0] = np.array([[1., 1., 4., 4., .9], [3.2, 2., 2.6, 5., .8]])          # rounds to x1 = 3, x2 = 3: fine; then x2 < x1
    boxes[1][0][1, 2] = 2.4
    with pytest.raises(ValueError, match=r'all_boxes\[1\]\[0\]: detection 1 has the box \[3, 2, 2, 5\] .* x2 < x1 or y2 < y1'):
        ev.convert_detections(boxes, masks)
    for bad_counts, words in (([-1, 1, 36], 'non-negative integers'), ([35.5, 0.5], 'non-negative integers'), ([1 << 32, 1], 'below 2\\^32')):
        with pytest.raises(ValueError, match=words):
            rle_counts({'size': [6, 6], 'counts': bad_counts}, 6, 6, 'x')
    p = Params()
    p.useSegm = 1
    with pytest.raises(NotImplementedError, match='useSegm'):          # the box evaluator keeps refusing it
        COCOBoxEvaluator({'image': [], 'category': [], 'bbox': [], 'area': [], 'iscrowd': []}, [1], [1], p)
    assert COCOSegmEvaluator(gt, *args, params=p).params.useSegm == 1
    p.useCats = 0
    with pytest.raises(NotImplementedError, match='useCats'):
        COCOSegmEvaluator(gt, *args, params=p)


def test_from_roidb_takes_run_length_encoded_masks(golden):
    from sniper_amd.evaluation import COCOSegmEvaluator
    d = golden['edge']
    roidb, num_classes = U.roidb_of(d)
    ev = COCOSegmEvaluator.from_roidb(roidb, num_classes)
    order = np.argsort(d['gt_image'], kind='stable')
    assert np.array_equal(ev.gt['image'], d['gt_image'][order]) and np.array_equal(ev.gt['category'], d['gt_category'][order])
    assert np.array_equal(ev.gt['area'], d['gt_area'][order]) and np.array_equal(ev.gt['iscrowd'], d['gt_iscrowd'][order] != 0)
    assert all(np.array_equal(a, d['gt_counts'][n]) for a, n in zip(ev.gt_rle, order))
    assert np.array_equal(ev.image_sizes, d['sizes']) and ev.cat_ids == [1, 2, 3]


def test_paste_boxes_clip_and_round_like_the_reference():
    """clip_boxes (bbox_transform.py:35-50) in float64, then np.round(...).astype(int): halves go to even, -0.4 clips to 0"""
    from sniper_amd.evaluation import paste_boxes
    rows = np.array([[-3.2, 1.5, 20.6, 8.5, .9], [0.5, 2.5, 3.5, 100., .8], [14.49, 0., 15.51, 9.4, .7]], np.float32)
    want = np.array([[0, 2, 15, 8], [0, 2, 4, 9], [14, 0, 15, 9]])
    got = paste_boxes(rows, 10, 16)
    assert got.dtype.kind == 'i' and np.array_equal(got, want)
    assert np.array_equal(rows[:, 0], np.array([-3.2, 0.5, 14.49], np.float32)), 'the caller\'s rows are not clipped in place'
    with pytest.raises(ValueError, match='detection 1 has the box .* y2 < y1'):
        paste_boxes(np.array([[1, 1, 3, 3, .5], [1, 5.6, 3, 5.4, .5]]), 10, 16, 'cell')


def test_resize_restatement_properties():
    """scale 1 is the identity, a constant mask stays constant where the coefficients are exact, the exact 2 x decimation is the
    block mean, and a 1 x 1 mask fills any box"""
    rng = np.random.RandomState(0)
    for M in (1, 14, 28):
        S = rng.rand(M, M).astype(np.float32)
        assert ref.resize_linear_f32(S, M, M).tobytes() == S.tobytes()
        out = ref.resize_linear_f32(S, 3 * M + 1, 2 * M + 5)
        assert out.shape == (3 * M + 1, 2 * M + 5) and out.dtype == np.float32 and out.min() >= S.min() and out.max() <= S.max()
        assert (ref.resize_linear_f32(np.full((M, M), 0.5, np.float32), 9, 31) == 0.5).all()
    S = rng.rand(14, 14).astype(np.float32)
    half = ref.resize_linear_f32(S, 7, 7)
    assert half[2, 3] == (((S[4, 6] + S[4, 7]) + S[5, 6]) + S[5, 7]) * np.float32(0.25)
    # (the y coefficient is not clamped: a 1 x 1 mask of 0.7 gives 0.7 * (1 - g) + 0.7 * g, not 0.7 itself; 0.5 scales exactly)
    assert (ref.resize_linear_f32(np.array([[0.5]], np.float32), 5, 9) == np.float32(0.5)).all()
    img = ref.paste(np.ones((14, 14), np.float32), [2, 1, 5, 3], 6, 8)
    assert [int(v) for v in img] == [13, 3, 3, 3, 3, 3, 3, 3, 14]
