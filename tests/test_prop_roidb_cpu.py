"""CPU: the numpy restatement of the reference's proposal roidb code (tests/prop_roidb_ref.py) equals what the reference's own
imdb.py returned (tests/golden/proproidb_v1.npz) on the bits, for every returned array and for the summary string, on all three
sets; its device-layout form says the same; and the host-only parts of sniper_amd.proposal_roidb (merge_roidbs, filter_roidb, the
chunking) do what the reference's do."""
import copy

import numpy as np
import pytest

import prop_roidb_ref as R
import prop_roidb_util as U


@pytest.fixture(scope='module')
def golden():
    return U.load_golden()


@pytest.fixture(scope='module')
def restated(golden):
    """per set: the kept rows, the proposal records and the merged roidb of the restatement, computed once"""
    out = {}
    for name, (s, _) in golden.items():
        kept = R.load_rpn_data(s['props'])
        rpn = R.create_roidb_from_box_list(kept, U.gt_roidb_of(s), s['num_classes'])
        merged = R.merge_roidbs(U.gt_roidb_of(s), copy.deepcopy(rpn))
        out[name] = (kept, rpn, merged)
    return out


def golden_kept(s, gold):
    idx = np.split(gold['keep_idx'], np.cumsum(gold['keep_counts'])[:-1])
    return [p[i] for p, i in zip(s['props'], idx)]


@pytest.mark.parametrize('name', U.SETS)
def test_restatement_equals_the_reference(golden, restated, name):
    s, gold = golden[name]
    kept, rpn, merged = restated[name]
    want = golden_kept(s, gold)
    assert len(kept) == len(want)
    for i, (a, b) in enumerate(zip(kept, want)):
        assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, 'load_rpn_data', i)
    got = {'max_overlaps': np.concatenate([r['max_overlaps'] for r in rpn] + [np.zeros(0, np.float32)]),
           'max_classes': np.concatenate([r['max_classes'] for r in rpn] + [np.zeros(0, np.int64)])}
    U.assert_same_bits(got, gold, ('max_overlaps', 'max_classes'), name)
    for r in rpn:      # the dense rows hold max_overlaps at max_classes and nothing else (what the golden file relies on)
        dense = np.zeros_like(r['gt_overlaps'])
        dense[np.arange(len(dense)), r['max_classes']] = r['max_overlaps']
        assert r['gt_overlaps'].dtype == np.float32 and r['gt_overlaps'].tobytes() == dense.tobytes()
        assert r['gt_classes'].dtype == np.int32 and not r['gt_classes'].any() and r['flipped'] is False
    assert [len(r['boxes']) for r in merged] == list(gold['merged_rows'])
    assert [len(r['proposal_scores']) for r in merged] == list(gold['merged_scores'])
    assert R.evaluate_recall(merged)['summary'] == gold['summary']
    assert R.evaluate_recall(merged, candidate_boxes=kept)['summary'] == gold['summary_cand']


def test_merge_keeps_the_references_quirk(golden):
    """imdb.py:417 looks 'proposal_scores' up in the lists: the proposals' scores are never appended"""
    _, gold = golden['coco_like']
    assert (gold['merged_scores'] < gold['merged_rows']).all()
    s, _ = golden['small']
    from sniper_amd import proposal_roidb as P
    rpn = R.create_roidb_from_box_list(R.load_rpn_data(s['props']), U.gt_roidb_of(s), s['num_classes'])
    mine, ref = P.merge_roidbs(U.gt_roidb_of(s), copy.deepcopy(rpn)), R.merge_roidbs(U.gt_roidb_of(s), copy.deepcopy(rpn))
    for a, b in zip(mine, ref):
        assert sorted(a) == sorted(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
            else:
                assert a[k] == b[k], k
        assert len(a['proposal_scores']) == len(a['boxes']) - len([1 for c in a['gt_classes'] if c == 0])
    # a ground-truth roidb without the dense rows (this project's) merges to one without
    bare = [{k: v for k, v in r.items() if k != 'gt_overlaps'} for r in U.gt_roidb_of(s)]
    assert all('gt_overlaps' not in r for r in P.merge_roidbs(bare, copy.deepcopy(rpn)))


@pytest.mark.parametrize('name', U.SETS)
def test_device_layout_form_says_the_same(golden, restated, name):
    s, gold = golden[name]
    kept, rpn, merged = restated[name]
    lay = U.nms_layout(s['props'])
    got = R.nms_ref(lay['rows'], lay['off'])
    assert list(got['nkeep']) == list(gold['keep_counts'])
    assert np.array_equal(np.concatenate([got['keep'][o:o + n] for o, n in zip(lay['off'][:-1], got['nkeep'])] + [np.zeros(0, np.int32)]),
                          gold['keep_idx'])
    assert (np.concatenate([got['keep'][o + n:e] for o, n, e in zip(lay['off'][:-1], got['nkeep'], lay['off'][1:])] + [np.zeros(0)]) == -1).all()
    a = U.assign_layout([k[:, :4] for k in kept], s['gt_boxes'], s['gt_classes'])
    got = R.assign_ref(a['boxes'], a['box_off'], a['gt'], a['gt_classes'], a['gt_off'])
    assert got['max_ov'].tobytes() == gold['max_overlaps'].tobytes()
    assert np.array_equal(np.where(got['max_ov'] > 0, got['max_cls'], 0), gold['max_classes'])
    r = U.recall_layout([k[:, :4] for k in kept], s['gt_boxes'], R.AREA_RANGES)
    got = R.recall_ref(r['boxes'], r['box_off'], r['gt'], r['gt_mask'], r['gt_off'], 7, R.default_thresholds())
    want = R.evaluate_recall(merged)
    assert np.array_equal(got['num_pos'], want['num_pos']) and np.array_equal(got['hits'], want['hits'])
    n = np.diff(r['box_off'])
    for a_ in range(7):
        cs = np.concatenate(([0], np.cumsum((r['gt_mask'] >> a_) & 1, dtype=np.int64)))
        vals = [got['gt_ov'][a_, o:o + cs[e] - cs[o]] for o, e, k in zip(r['gt_off'][:-1], r['gt_off'][1:], n) if k > 0]
        assert np.sort(np.concatenate(vals + [np.zeros(0)])).tobytes() == want['gt_overlaps'][a_].tobytes()


def test_equal_scores_rank_the_later_row_first():
    rows = np.array([[0, 0, 9, 9, .5], [1, 0, 10, 9, .5], [50, 50, 59, 59, .5]], np.float32)      # rows 0 and 1 overlap (IoU 0.82)
    assert R.nmsp(rows) == [2, 1]
    assert R.nmsp(rows[::-1].copy()) == [2, 0]


def test_edges_hold_what_they_are_made_for(golden):
    s, gold = golden['edges']
    keep = np.split(gold['keep_idx'], np.cumsum(gold['keep_counts'])[:-1])
    assert sorted(keep[6]) == [0, 1]                            # float32 IoU exactly 7 / 10: `<=` keeps the pair
    inter = np.float32(70)
    assert inter / (np.float32(100) + np.float32(70) - inter) == np.float32(0.7)
    assert R.bbox_overlaps(s['props'][7][:, :4], s['gt_boxes'][7])[0, 0] == 0.5
    m = U.area_masks(s['gt_boxes'], R.AREA_RANGES)[8]
    assert m[0] == 0b101                                        # area 625: `all` and 25-50, not 0-25
    ov = R.bbox_overlaps(s['props'][4][:, :4], s['gt_boxes'][4])
    assert ov[0, 0] == ov[0, 1] > 0
    assert list(R.greedy_match(ov)) == [ov[0, 0], 0.0]          # the lower row takes the box, the other is left with the far box


def test_filter_and_chunks():
    from sniper_amd import config as cfgmod
    from sniper_amd import proposal_roidb as P
    cfg = cfgmod.res101_e2e(batch_images=4)
    roidb = [{'max_overlaps': np.array([1.0, 0.3], np.float32)}, {'max_overlaps': np.zeros(0, np.float32)}]
    assert P.filter_roidb(roidb, cfg) == roidb[:1]
    ev = P.ProposalRoidbEvaluator.__new__(P.ProposalRoidbEvaluator)
    ev.chunk_bytes = 100
    assert ev._chunks([40, 40, 40, 300, 10, 0, 90]) == [(0, 2), (2, 3), (3, 4), (4, 7)]
    assert ev._chunks([]) == []
    ev.max_gt = 5
    with pytest.raises(ValueError, match=r'image 1 \(b\.jpg\) has 6 ground-truth boxes'):
        ev.check_gt([5, 6], names=['a.jpg', 'b.jpg'])
