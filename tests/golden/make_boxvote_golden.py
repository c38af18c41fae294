"""Generate tests/golden/boxvote_v1.npz with the REFERENCE's own compiled bbox_overlaps_cython (build container only; the GPU box
and the test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_boxvote_golden.py

Box voting is this project's operator; what it shares with the reference is who votes for whom:
`bbox_overlaps_cython(top, all) >= thresh` of lib/bbox/bbox.pyx, which oracle.build compiles into oracle/_ref/ from the source where
it lies.  The file pins those vote sets to the reference's arithmetic, not to the restatement in tests/box_vote_ref.py.

What the file holds -- arrays only: the sets of box_vote_ref.golden_inputs() and three fixed edge sets (the pair at IoU exactly 0.5,
exact duplicates, a degenerate box), stacked
  all_rows (sum n_a, 5) f32, all_sizes (S,)     the pre-NMS rows of every set
  top_rows (sum n_t, 5) f32, top_sizes (S,)     the kept rows
  member_50 / member_80 / member_100            np.packbits of the (n_t, n_a) vote sets of every set, back to back, per threshold
  nonneg (S,) u8                                1 for the sets whose coordinates are all >= 0

Conditions asserted, so that a test cannot pass without testing anything (on the reference's output): over the clustered sets at
least half of the kept rows have two or more voters at 0.5 and at 0.8, and at least one voted coordinate differs from its input;
the IoU 0.5 pair votes at 0.5 and the 0.4 box does not; the degenerate box has no voter, itself included."""
import glob
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import box_vote_ref as R  # noqa: E402
from oracle import build  # noqa: E402

GOLDEN = os.path.join(HERE, 'boxvote_v1.npz')


def load_reference():
    build.build_reference()
    ext = glob.glob(os.path.join(build.REF_OUT, 'bbox*.so'))
    assert len(ext) == 1, ext
    spec = importlib.util.spec_from_file_location('bbox', ext[0])
    mod = importlib.util.module_from_spec(spec)
    alias = not hasattr(np, 'float')
    if alias:
        np.float = float      # bbox.pyx:14 spells its dtype with the alias numpy dropped; only while the extension initialises
    try:
        spec.loader.exec_module(mod)
    finally:
        if alias:
            del np.float
    return mod.bbox_overlaps_cython


def main():
    assert build.have_reference(), 'the reference is not here: this script runs in the build container only'
    overlaps = load_reference()
    edges = R.problem_sets(64, 128)
    sets = R.golden_inputs() + [edges[k] for k in ('IoU exactly 0.5', 'duplicates', 'degenerate')]
    n_clustered = len(sets) - 3
    member = {t: [] for t in R.THRESHOLDS}
    two, rows, moved = {t: 0 for t in R.THRESHOLDS}, 0, 0
    for k, (top, alld) in enumerate(sets):
        ov = overlaps(np.ascontiguousarray(top[:, :4], np.float64), np.ascontiguousarray(alld[:, :4], np.float64))
        assert ov.dtype == np.float64 and ov.shape == (len(top), len(alld))
        for t in R.THRESHOLDS:
            m = ov >= t
            member[t].append(m.ravel())
            if k < n_clustered:
                two[t] += int((m.sum(1) >= 2).sum())
                moved += int((R.box_vote_ref(top, alld, t, 'ID', ov=ov, member=m)[:, :4] != top[:, :4]).sum())
        rows += len(top) if k < n_clustered else 0
        if k == n_clustered:
            assert ov[0, 1] == 0.5 and ov[0, 2] == 0.4 and list(ov[0] >= 0.5) == [True, True, False]
        if k == n_clustered + 2:
            assert not (ov[0] > 0).any()
    for t in (0.5, 0.8):
        print('thresh %.1f: %d of %d kept rows have two or more voters' % (t, two[t], rows))
        assert 2 * two[t] >= rows, (t, two[t], rows)
    assert moved > 0
    out = {'all_rows': np.concatenate([a for _, a in sets]), 'all_sizes': np.array([len(a) for _, a in sets], np.int32),
           'top_rows': np.concatenate([t for t, _ in sets]), 'top_sizes': np.array([len(t) for t, _ in sets], np.int32),
           'nonneg': np.array([int((a[:, :4] >= 0).all()) for _, a in sets], np.uint8)}
    for t in R.THRESHOLDS:
        out['member_%d' % round(100 * t)] = np.packbits(np.concatenate(member[t]))
    np.savez_compressed(GOLDEN, **out)
    print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes;', len(sets), 'sets,', int(out['all_sizes'].sum()), 'rows')
    assert os.path.getsize(GOLDEN) <= 316525, 'larger than the largest golden file so far'


if __name__ == '__main__':
    main()
