"""CPU: the inputs of tests/test_gpu_roi_pool_paths.py reach the kernel branches their cases name, shown without a GPU by the
numpy restatement of the bin geometry (tests/roi_paths_util.py), and that restatement agrees with oracle/nn.py."""
import numpy as np
import pytest

import roi_paths_util as rp
from oracle import nn as onn


@pytest.mark.parametrize('case', rp.DPSROI_CASES + rp.PSROI_CASES, ids=repr)
def test_case_reaches_its_window_classes_without_rounding_dependent_samples(case):
    assert case.check_reach()
    n = [rp.class_counts(case.paths(t)) for t, _ in case.modes]
    print(case.name, n)
    if case.G == 1:
        # the kernel family: pooled * pooled <= 64 takes the per-RoI kernels and the MFMA data gradient, the generic ones beyond
        assert (case.P * case.P > rp.K_BINS_MAX) == case.name.startswith('generic')
    assert case.R * case.P * case.P * case.S * case.S <= 400000 and max(case.H, case.W) <= 80
    # a region of the map no RoI touches (the data gradient must be exactly zero there), unless the case says it has none
    rois, trans = case.inputs()
    for with_trans, tstd in case.modes:
        free = rp.untouched_cells(rois, trans if with_trans else None, case.B, case.H, case.W, case.P, case.S, 1.0 / rp.SC, tstd)
        assert free.any() or case.dense, (case.name, with_trans)


def test_named_cases_hold_what_their_rows_are_there_for():
    by = {c.name: c for c in rp.DPSROI_CASES + rp.PSROI_CASES}
    for t in (False, True):
        # every class, in the per-RoI kernels; oversized and 5-8 windows at S = 4, at S = 8 and in the position-sensitive kernels
        assert min(rp.class_counts(by['roi-P2-all-classes'].paths(t)).values()) > 0
        for name in ('roi-P7-large-map', 'roi-P8-S8-large-map', 'ps-D40-S4', 'ps-D5-S8'):
            n = rp.class_counts(by[name].paths(t))
            assert n['>8'] >= 9 and n['5-8'] > 0, (name, n)
        # the generic kernels' large windows: 5 - 8 cells
        assert rp.class_counts(by['generic-P14-large-map'].paths(t))['5-8'] >= 100
        # a 5-8 window with more than 4 cells on ONE axis only: the rolled loop's second half of the weight table on that axis
        p = by['roi-P7-large-map'].paths(t)
        mid = p['cls'] == rp.CLASSES.index('5-8')
        assert (p['nx'][mid] > 4).any() and (p['ny'][mid] > 4).any()
    # P * P = 64 with more than 256 RoIs: two scan rounds of the tile-owner kernel
    c = by['mfma-P8-R300']
    assert c.P * c.P == rp.K_BINS_MAX and c.R > 256
    assert by['mfma-C512'].C == 512 and by['mfma-C24'].C % 64 != 0 and not by['mfma-C24'].with_trans
    assert by['roi-S1-C8'].C // 8 == 1 and by['roi-S1-C8'].S == 1
    assert by['generic-P16-S2'].P == 16
    assert by['ps-D40-S4'].C >= 32 > by['ps-D5-S8'].C


def test_helper_counts_equal_the_oracles():
    """Valid-sample count per bin against oracle/nn.py: sample for sample against the loop statement's rule (_roi_bins and the
    validity test of dpsroi_pool), and through _dpsroi_operators, whose rows sum to 1 where a bin has a sample and to 0 where
    not (the bilinear weights of a sample sum to 1, the row is their mean over the valid samples)."""
    case = [c for c in rp.DPSROI_CASES if c.name == 'roi-S1-C8'][0]
    small = rp.PoolCase('small', 2, 8, 9, 11, 12, 3, 4, ())
    for c in (case, small):
        rois, trans = c.inputs()
        for tr, tstd in ((None, 0.0), (trans, rp.TRANS_STD)):
            p = rp.bin_paths(rois, tr, c.P, c.S, 1.0 / rp.SC, tstd, c.H, c.W)
            want = np.zeros((c.R, c.P, c.P), np.int64)
            lo = np.full((2, c.R, c.P, c.P), 10 ** 6)
            hi = np.full((2, c.R, c.P, c.P), -1)
            for r in range(c.R):
                for ph in range(c.P):
                    for pw in range(c.P):
                        ws, hs, sw_, sh_, _, _ = onn._roi_bins(rois[r], tr, r, ph, pw, c.P, c.S, 1.0 / rp.SC, tstd)
                        for ih in range(c.S):
                            for iw in range(c.S):
                                w, h = ws + iw * sw_, hs + ih * sh_
                                if w < -0.5 or w > c.W - 0.5 or h < -0.5 or h > c.H - 0.5:
                                    continue
                                want[r, ph, pw] += 1
                                w, h = min(max(w, 0.0), c.W - 1.0), min(max(h, 0.0), c.H - 1.0)
                                lo[0, r, ph, pw] = min(lo[0, r, ph, pw], int(np.floor(w)))
                                hi[0, r, ph, pw] = max(hi[0, r, ph, pw], int(np.ceil(w)))
                                lo[1, r, ph, pw] = min(lo[1, r, ph, pw], int(np.floor(h)))
                                hi[1, r, ph, pw] = max(hi[1, r, ph, pw], int(np.ceil(h)))
            assert p['ambiguous'] == 0
            assert np.array_equal(p['count'], want) and np.array_equal(p['count_oracle'], want)
            assert (want == 0).any() and (want == c.S * c.S).any() and (c.S == 1 or ((want > 0) & (want < c.S * c.S)).any())
            has = want > 0
            assert np.array_equal(p['nx'][has], (hi[0] - lo[0] + 1)[has]) and np.array_equal(p['ny'][has], (hi[1] - lo[1] + 1)[has])
            assert (p['nx'][~has] == 0).all() and (p['ny'][~has] == 0).all()
            A = onn._dpsroi_operators(rois, tr, c.B, c.H, c.W, c.P, c.S, 1.0 / rp.SC, tstd)[0]
            rows = np.asarray(A.sum(1)).reshape(c.R, c.P, c.P)
            assert np.allclose(rows, (want > 0).astype(np.float64), atol=1e-12)
            # and the cells of a bin's window are the columns of its row
            for r, ph, pw in ((0, 0, 0), (1, c.P - 1, c.P - 1), (5, 1, 0)):
                cols = A[(r * c.P + ph) * c.P + pw].nonzero()[1]
                if not len(cols):
                    assert not has[r, ph, pw]
                    continue
                b = int(rois[r, 0])
                ys, xs = (cols // c.W) - b * c.H, cols % c.W
                assert p['x_lo'][r, ph, pw] <= xs.min() and xs.max() <= p['x_hi'][r, ph, pw]
                assert p['y_lo'][r, ph, pw] <= ys.min() and ys.max() <= p['y_hi'][r, ph, pw]


def test_ambiguous_samples_are_flagged():
    """A sample that fmaf(i, sub, start) and start + float32(i) * sub put on different sides of a cell boundary, or of the
    validity edge dim - 0.5, is reported, and one they agree on is not: starts chosen so that sample 7 lands within an ulp of
    an integer (of 63.5 for the edge)."""
    rs = np.random.RandomState(0)
    i, dim, found_cell, found_edge, clean = 7, 64, 0, 0, 0
    for target in (17.0, 63.5):
        for _ in range(3000):
            sub = np.float32(rs.uniform(0.05, 12))
            start = np.float32(target - np.float64(i) * np.float64(sub))
            fused = np.float32(np.float64(i) * np.float64(sub) + np.float64(start))
            split = np.float32(start + np.float32(i) * sub)
            amb = rp._axis(np.full((1, 1, 1), start, np.float32), np.array([sub], np.float32), 8, dim)[4][0, 0, 0]
            ok_f, ok_s = not (fused < -0.5 or fused > dim - 0.5), not (split < -0.5 or split > dim - 0.5)
            differs = ok_f != ok_s or (ok_f and (np.floor(fused) != np.floor(split) or np.ceil(fused) != np.ceil(split)))
            assert bool(amb[i]) == bool(differs), (start, sub, fused, split)
            if differs:
                found_cell += target == 17.0
                found_edge += target == 63.5
            else:
                clean += 1
    assert found_cell > 0 and found_edge > 0 and clean > 0, (found_cell, found_edge, clean)


def test_deform_candidate_window_contains_every_reachable_row():
    """The restated candidate window (what the GPU test compares its pruning claim with) is conservative: every output row that
    can reach a tile under |offset| <= dmax is inside it, for the strides, pads, dilations and kernel spans of the GPU cases."""
    for (KH, KW, stride, pad, dil) in ((3, 3, 2, 1, 1), (3, 3, 2, 2, 2), (1, 1, 1, 0, 1), (1, 3, 1, 1, 1), (3, 3, 1, 2, 2)):
        for dim in (12, 14):
            dim_out = rp.deform_out_size(dim, dim, KH, KW, stride, pad, dil)[0]
            for dmax in (0.0, 0.75, 1.0, 2.5):
                for t0 in range(0, dim, 4):
                    lo, hi = rp.deform_candidate_range(t0, dim_out, dmax, KH, KW, stride, pad, dil)
                    for o in range(dim_out):
                        for k in range(max(KH, KW)):
                            base = o * stride - pad + k * dil
                            if base + dmax >= t0 - 1 and base - dmax < t0 + 4:
                                assert lo <= o <= hi, (KH, KW, stride, pad, dil, dim, dmax, t0, o, k, lo, hi)
