"""GPU: the proposal roidb kernels (csrc/prop_roidb.hip) and sniper_amd.proposal_roidb against the reference's own output
(tests/golden/proproidb_v1.npz) and the numpy restatement (tests/prop_roidb_ref.py).  Every comparison is on the bits: every float
operation is restated in the reference's precision and order, and the only accumulation across workgroups is integer."""
import copy
import os
import pickle

import numpy as np
import pytest

import prop_roidb_ref as R
import prop_roidb_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    return U.load_golden()


def golden_kept(s, gold):
    idx = np.split(gold['keep_idx'], np.cumsum(gold['keep_counts'])[:-1])
    return [p[i] for p, i in zip(s['props'], idx)]


def layouts(props, boxes_list, gt_boxes, gt_classes, area_ranges=R.AREA_RANGES):
    return (U.nms_layout(props), U.assign_layout(boxes_list, gt_boxes, gt_classes), U.recall_layout(boxes_list, gt_boxes, area_ranges))


_REF = {}


def set_case(golden, name):
    """a golden set's three layouts (assignment and recall on the rows the reference kept) and their restatement, computed once"""
    if name not in _REF:
        s, gold = golden[name]
        lay = layouts(s['props'], [k[:, :4] for k in golden_kept(s, gold)], s['gt_boxes'], s['gt_classes'])
        _REF[name] = (lay, U.restatement(*lay, R.default_thresholds()))
    return _REF[name]


@pytest.mark.parametrize('name', U.SETS)
def test_device_equals_golden_and_restatement(golden, name):
    s, gold = golden[name]
    lay, want = set_case(golden, name)
    got = U.device_run(*lay, R.default_thresholds())
    U.assert_same_bits(got, want, U.DEVICE_KEYS, name)
    again = U.device_run(*lay, R.default_thresholds())
    for k in U.DEVICE_KEYS:
        assert got[k].tobytes() == again[k].tobytes(), (name, k, 'two runs differ')
    off = lay[0]['off']
    assert np.array_equal(got['nkeep'], gold['keep_counts'])
    assert np.array_equal(np.concatenate([got['keep'][o:o + n] for o, n in zip(off[:-1], got['nkeep'])] + [np.zeros(0, np.int32)]),
                          gold['keep_idx'])
    assert got['max_ov'].tobytes() == gold['max_overlaps'].tobytes()
    assert np.array_equal(np.where(got['max_ov'] > 0, got['max_cls'], 0), gold['max_classes'])


@pytest.mark.parametrize('name', U.SETS)
def test_python_surface_equals_golden(golden, name, capsys):
    """nms_proposals, proposal_roidb and evaluate_recall (candidate_boxes taken from the roidb's non-GT rows, and given)"""
    from sniper_amd import proposal_roidb as P
    s, gold = golden[name]
    kept = P.nms_proposals(s['props'])
    for a, b in zip(kept, golden_kept(s, gold)):
        assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
    merged = P.proposal_roidb(U.gt_roidb_of(s), kept, s['num_classes'], append_gt=True)
    want = R.merge_roidbs(U.gt_roidb_of(s), R.create_roidb_from_box_list(kept, U.gt_roidb_of(s), s['num_classes']))
    assert_same_roidb(merged, want)
    assert [len(r['proposal_scores']) for r in merged] == list(gold['merged_scores'])
    for cand, key in ((None, 'summary'), (kept, 'summary_cand')):
        capsys.readouterr()
        res = P.evaluate_recall(merged, candidate_boxes=cand)
        assert res.summary() == gold[key]
        assert capsys.readouterr().out == ''.join(ln + '\n' for ln in res.lines)          # printed, as the reference prints them
        ref = R.evaluate_recall(want, candidate_boxes=cand)
        assert np.array_equal(res.area_counts, ref['area_counts']) and np.array_equal(res.num_pos, ref['num_pos'])
        assert np.array_equal(res.hits, ref['hits'])
        assert U.same_bits(res.recalls, ref['recalls']) and U.same_bits(res.ar, ref['ar'])
        for a, b in zip(res.gt_overlaps, ref['gt_overlaps']):
            assert a.dtype == np.float64 and a.tobytes() == b.tobytes()


def assert_same_roidb(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b), (i, sorted(a), sorted(b))
        for k in a:
            if isinstance(b[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (i, k)
            else:
                assert a[k] == b[k], (i, k)


def test_size_seams():
    """N on both sides of every block seam crossed with G up to the limit, all pairs in one call"""
    lim = U.limits()
    B, gmax = lim['assign_block'], lim['max_gt']
    assert lim['recall_threads'] == B and lim['sort_tile'] == B and B % lim['nms_tile'] == 0
    pairs = [(n, g) for g in (0, 1, 63, 64, 65, gmax) for n in (0, 1, B - 1, B, B + 1, 2 * B + 1)]
    props, gts, classes = U.seam_problems(7, pairs)
    assert sum(len(p) for p in props) < 20000
    lay = layouts(props, [p[:, :4] for p in props], gts, classes)
    assert all(((lay[2]['gt_mask'] >> a) & 1).any() for a in range(7))            # every range has rows
    got = U.device_run(*lay, R.default_thresholds())
    U.assert_same_bits(got, U.restatement(*lay, R.default_thresholds()), U.DEVICE_KEYS, 'seams')
    assert 0 < got['nkeep'].sum() < len(lay[0]['rows']) and got['hits'][0, 0] > got['hits'][0, -1] > 0


def test_too_many_ground_truth_boxes_is_refused_before_any_launch(monkeypatch):
    from sniper_amd import hip
    from sniper_amd import proposal_roidb as P
    gmax = P.limits()['max_gt']
    props, gts, classes = U.seam_problems(8, [(5, 3), (4, gmax + 1)])
    gt_roidb = [{'image': 'im%d.jpg' % i, 'height': 600, 'width': 600, 'boxes': g, 'gt_classes': c} for i, (g, c) in enumerate(zip(gts, classes))]

    def no_launch(name, *args):
        raise AssertionError('%s was called' % name)
    monkeypatch.setattr(hip, 'call', no_launch)
    with pytest.raises(ValueError, match=r'image 1 \(im1\.jpg\) has %d ground-truth boxes' % (gmax + 1)):
        P.proposal_roidb(gt_roidb, props, 81, append_gt=False)
    roidb = [{'boxes': np.vstack((g, p[:, :4])), 'gt_classes': np.concatenate((c, np.zeros(len(p), np.int32))),
              'max_overlaps': np.concatenate((np.ones(len(g), np.float32), np.zeros(len(p), np.float32))), 'image': 'im%d.jpg' % i}
             for i, (p, g, c) in enumerate(zip(props, gts, classes))]
    with pytest.raises(ValueError, match=r'image 1 \(im1\.jpg\)'):
        P.evaluate_recall(roidb)


def test_nms_tie_rule():
    """images of equal scores (all equal; four values): the later row of equal score ranks first, as the restatement's
    argsort(kind='stable')[::-1]"""
    props, gts, classes = U.seam_problems(9, [(300, 4), (300, 4), (70, 1)])
    props[0][:, 4] = 0.5
    props[1][:, 4] = (np.arange(300) % 4 / 4.0).astype(np.float32)
    props[2][:, 4] = 0.25
    lay = layouts(props, [p[:, :4] for p in props], gts, classes)
    got = U.device_run(*lay, [0.5])
    want = R.nms_ref(lay[0]['rows'], lay[0]['off'])
    U.assert_same_bits(got, want, ('keep', 'nkeep'), 'ties')
    assert got['keep'][0] == 299 and got['keep'][lay[0]['off'][2]] == 69          # the last row of an all-equal image is kept first
    # the opposite rule gives another answer on this input: the test can fail
    first = R.nmsp(props[0][::-1].copy())
    assert [299 - k for k in first] != list(got['keep'][:got['nkeep'][0]])


@pytest.mark.parametrize('T', (1, 10))
@pytest.mark.parametrize('A', (1, 7))
def test_thresholds_and_ranges(golden, A, T):
    lay, want = set_case(golden, 'coco_like')
    s, gold = golden['coco_like']
    thrs = R.default_thresholds()[:T]
    rec_lay = U.recall_layout([k[:, :4] for k in golden_kept(s, gold)], s['gt_boxes'], R.AREA_RANGES[:A])
    got = U.device_run(lay[0], lay[1], rec_lay, thrs)
    assert got['hits'].shape == (A, T) and got['gt_ov'].shape == (A, len(rec_lay['gt']))
    assert np.array_equal(got['hits'], want['hits'][:A, :T]) and np.array_equal(got['num_pos'], want['num_pos'][:A])
    assert got['gt_ov'].tobytes() == want['gt_ov'][:A].tobytes()


def test_closed_loop_trains_with_negative_chips(tmp_path, capsys):
    """pickle -> rpn_roidb(append_gt=True) -> filter_roidb -> one MNIteratorE2E reset with TRAIN.USE_NEG_CHIPS: the roidb is the
    restatement's array by array, the second call reads the cache the first wrote, and negative chips are mined from it"""
    from sniper_amd import config as cfgmod
    from sniper_amd import proposal_roidb as P
    from sniper_amd.iterators import MNIteratorE2E
    from sniper_amd.synthetic import make_roidb
    s = U.coco_like_set(n_images=8, seed=11)
    gt = lambda: make_roidb(8, seed=11, num_classes=81)
    for rec, boxes in zip(gt(), s['gt_boxes']):
        assert np.array_equal(rec['boxes'], boxes)

    class Imdb(P.ProposalRoidbMixin):
        name, num_classes, num_images = 'synthetic_train', 81, 8
    path = str(tmp_path)
    with open(os.path.join(path, 'synthetic_train_rpn.pkl'), 'wb') as fh:
        pickle.dump(s['props'], fh, pickle.HIGHEST_PROTOCOL)
    roidb = Imdb().rpn_roidb(gt(), append_gt=True, proposal_path=path)
    cache = os.path.join(path, 'synthetic_train_rpn_after_nms.pkl')
    with open(cache, 'rb') as fh:
        boxes, maps = pickle.load(fh)
    assert maps == [] and len(boxes) == 8
    kept = R.load_rpn_data(s['props'])
    for a, b in zip(boxes, kept):
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    want = R.merge_roidbs(gt(), R.create_roidb_from_box_list(kept, gt(), 81))
    assert_same_roidb(roidb, want)
    os.remove(os.path.join(path, 'synthetic_train_rpn.pkl'))          # the second call has only the cache to read
    capsys.readouterr()
    assert_same_roidb(Imdb().rpn_roidb(gt(), append_gt=True, proposal_path=path), want)
    assert 'Reading cached proposals after ***NMS****' in capsys.readouterr().out
    cfg = cfgmod.res101_e2e(batch_images=4)
    cfg.TRAIN.USE_NEG_CHIPS = True
    roidb = P.filter_roidb(roidb, cfg)
    assert len(roidb) == 8 and all((r['max_overlaps'][len(g):] < 1).all() for r, g in zip(roidb, s['gt_boxes']))
    np.random.seed(5)
    it = MNIteratorE2E(copy.deepcopy(roidb), cfg, batch_size=4, nGPUs=1, im_source='synthetic')
    assert sum(len(r['neg_crops']) for r in it.roidb) >= 1
    assert len(it) % 4 == 0 and it.batch is not None
