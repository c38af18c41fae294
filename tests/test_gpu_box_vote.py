"""GPU: sn_box_vote against the sequential restatement (tests/box_vote_ref.py), BIT for bit: float64 sums in ascending row order,
one divide, one narrowing -- nothing to tolerate.  Every scoring method, thresholds 0.5 / 0.8 / 1.0, the sizes at which the
kernel changes path (rows per tile, rows per LDS chunk, both taken from sn_box_vote_limits), and the vote sets the reference's own
bbox_overlaps_cython gave (tests/golden/boxvote_v1.npz)."""
import numpy as np
import pytest
import torch

import box_vote_ref as R
from gpu_util import dev
from test_box_vote_cpu import golden_sets

pytestmark = pytest.mark.gpu

_CACHE = {}


def _limits():
    from sniper_amd.ext import box_vote
    return box_vote.limits()


def _edge():
    """the edge set and its overlaps, computed once and left unchanged"""
    if 'edge' not in _CACHE:
        lim = _limits()
        sets = R.problem_sets(lim['tile'], lim['chunk'])
        _CACHE['edge'] = (sets, {k: R.overlaps(t, a) for k, (t, a) in sets.items()})
    return _CACHE['edge']


def _ragged():
    if 'ragged' not in _CACHE:
        probs = R.ragged_batch(40)
        _CACHE['ragged'] = (probs, [R.overlaps(t, a) for t, a in probs])
    return _CACHE['ragged']


def _run(problems, thresh, method, on_device=False):
    """one launch over the stacked problems -> (voted top_rows, the inputs)"""
    from sniper_amd.ext import box_vote
    top_rows, counts, all_rows, sizes = R.stack(problems)
    if not on_device:
        return box_vote.box_vote_stacked(top_rows, counts, all_rows, sizes, thresh, method), (top_rows, counts, all_rows, sizes)
    d_top, d_all = torch.from_numpy(top_rows).to(dev()), torch.from_numpy(all_rows).to(dev())
    d_cnt = torch.from_numpy(counts).to(dev())
    out = box_vote.box_vote_stacked(d_top, d_cnt, d_all, sizes, thresh, method)
    assert out is d_top and np.array_equal(d_all.cpu().numpy(), all_rows)              # in place; the voters are read only
    return out.cpu().numpy(), (top_rows, counts, all_rows, sizes)


def _want(problems, ovs, thresh, method):
    top_rows, counts, all_rows, sizes = R.stack(problems)
    off = np.concatenate(([0], np.cumsum(sizes)))
    for q, ((t, a), ov) in enumerate(zip(problems, ovs)):
        top_rows[off[q]:off[q] + len(t)] = R.box_vote_ref(t, a, thresh, method, ov=ov)
    return top_rows


def test_limits():
    lim = _limits()
    assert lim['tile'] >= 2 and lim['chunk'] >= 2


@pytest.mark.parametrize('thresh', R.THRESHOLDS)
@pytest.mark.parametrize('method', R.METHODS)
def test_edge_set_is_bit_equal_to_the_restatement(method, thresh):
    sets, ovs = _edge()
    lim = _limits()
    names = sorted(sets)
    problems = [sets[k] for k in names]
    got, (top_rows, counts, all_rows, sizes) = _run(problems, thresh, method)
    want = _want(problems, [ovs[k] for k in names], thresh, method)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), [
        k for k, a, b in zip(names, np.split(got, np.cumsum(sizes)[:-1]), np.split(want, np.cumsum(sizes)[:-1])) if a.tobytes() != b.tobytes()]
    off = dict(zip(names, np.concatenate(([0], np.cumsum(sizes)))))

    def rows(k):
        return got[off[k]:off[k] + len(sets[k][0])], sets[k][0]
    # what the sets are for (asserted on the inputs / the restatement, so that none of them passes by testing nothing)
    stale = np.ones(len(got), bool)
    for k in names:
        stale[off[k]:off[k] + len(sets[k][0])] = False
    assert stale.sum() > 100 and (got[stale] == np.float32(-12345.0)).all()          # rows past the count stay untouched
    for k in ('degenerate', 'zero scores'):
        g, t = rows(k)
        assert np.array_equal(g[0], t[0]) if k == 'degenerate' else np.array_equal(g, t)
    g, t = rows('IoU exactly 0.5')
    a = sets['IoU exactly 0.5'][1].astype(np.float64)
    if thresh == 0.5:             # rows 0 and 1 vote, the 0.4 box does not
        assert g[0, 3] == np.float32((a[0, 4] * a[0, 3] + a[1, 4] * a[1, 3]) / (a[0, 4] + a[1, 4])) and g[0, 2] == 9
    else:
        assert np.array_equal(g[:, :4], t[:, :4])
    g, t = rows('duplicates')
    assert np.array_equal(g[:, :4], t[:, :4])                     # the mean of equal boxes is the box, exactly, at every weight
    if method == 'AVG':
        assert g[0, 4] == np.float32(sets['duplicates'][1][:, 4].astype(np.float64).cumsum()[-1] / 5)
    g, t = rows('negative coordinates')
    assert (t[:, :4] < 0).any() and (g[:, :4] != t[:, :4]).any() == (thresh < 1.0)
    chunk = lim['chunk']
    m = ovs['n_a = %d' % (chunk + 1)] >= 0.5
    assert (m[:, :chunk].any(1) & m[:, chunk:].any(1)).any()      # a kept row with voters on both sides of the chunk boundary
    for n_t in (lim['tile'] - 1, lim['tile'], lim['tile'] + 1):
        assert len(sets['n_t = %d' % n_t][0]) == n_t
    if thresh < 1.0:
        voters = np.concatenate([(ovs[k] >= thresh).sum(1) for k in names if k.startswith('n_') and len(sets[k][0])])
        assert 2 * (voters >= 2).sum() >= len(voters)             # the clustered sets: most kept rows have company


@pytest.mark.parametrize('method', R.METHODS)
def test_ragged_batch_of_forty_problems(method):
    problems, ovs = _ragged()
    sizes = [len(a) for _, a in problems]
    assert len(problems) == 40 and sizes.count(0) >= 5 and sum(1 for t, a in problems if len(a) and not len(t)) >= 2
    for thresh in R.THRESHOLDS:
        got, _ = _run(problems, thresh, method, on_device=True)
        want = _want(problems, ovs, thresh, method)
        assert got.tobytes() == want.tobytes(), thresh
    voters = np.concatenate([(ov >= 0.8).sum(1) for (t, _), ov in zip(problems, ovs) if len(t)])
    assert 2 * (voters >= 2).sum() >= len(voters)                 # a test where nobody votes shows nothing
    top_rows = R.stack(problems)[0]
    assert (want[:, :4] != top_rows[:, :4]).sum() == 0            # thresh 1.0: only exact duplicates vote, nothing moves
    assert (_want(problems, ovs, 0.8, method)[:, :4] != top_rows[:, :4]).any()


def test_the_same_bits_every_run():
    problems, _ = _ragged()
    a, _ = _run(problems, 0.5, 'IOU_AVG', on_device=True)
    b, _ = _run(problems, 0.5, 'IOU_AVG', on_device=True)
    assert a.tobytes() == b.tobytes()


def test_one_problem_call_with_detectrons_signature():
    from sniper_amd.ext import box_vote
    top, alld = R.golden_inputs()[0]
    got = box_vote.box_voting(top, alld, 0.8, scoring_method='IOU_AVG')
    assert got.shape == top.shape and got.tobytes() == R.box_vote_ref(top, alld, 0.8, 'IOU_AVG').tobytes()
    assert box_vote.box_voting(np.zeros((0, 5)), alld, 0.8).shape == (0, 5)
    with pytest.raises(ValueError):
        box_vote.box_voting(alld, top, 0.8)                        # more kept boxes than boxes


@pytest.mark.parametrize('thresh', R.THRESHOLDS)
def test_vote_sets_are_the_references(thresh):
    """The vote sets come from the reference's own compiled overlap (the golden file): the device's 'AVG' score is
    (float)(den / |V|) and its coordinates (float)(num / den), both rebuilt here from the golden membership alone."""
    sets = golden_sets()
    problems = [(t, a) for t, a, _, _ in sets]
    got, (_, _, _, sizes) = _run(problems, thresh, 'AVG')
    off = np.concatenate(([0], np.cumsum(sizes)))
    rows = two = moved = 0
    for q, (top, alld, member, _) in enumerate(sets):
        want = R.box_vote_ref(top, alld, thresh, 'AVG', ov=np.zeros((len(top), len(alld))), member=member[thresh])
        g = got[off[q]:off[q] + len(top)]
        assert g.tobytes() == want.tobytes(), q
        den = np.array([alld[m, 4].astype(np.float64).cumsum()[-1] if m.any() else 0.0 for m in member[thresh]])
        n_v = member[thresh].sum(1)
        ok = (n_v > 0) & (den > 0)
        assert np.array_equal(g[ok, 4], (den[ok] / n_v[ok]).astype(np.float32))
        rows += len(top)
        two += int((n_v >= 2).sum())
        moved += int((g[:, :4] != top[:, :4]).sum())
    if thresh < 1.0:
        assert 2 * two >= rows and moved > 0
