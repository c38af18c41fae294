"""Which branch of csrc/roi_deform.hip an input reaches, restated on the CPU (plain numpy, float32 like the kernels), and the
inputs of tests/test_gpu_roi_pool_paths.py.  The kernels pick their inner path per (RoI, bin) from the cell window the bin's
valid samples span (dpsroi_fwd_roi_kernel: unrolled 2 / 3 / 4-cell windows, a rolled loop up to kWinMax = 8 cells per axis, the
on-the-fly path beyond), so a test that claims to cover a path has to show that its inputs get there:
tests/test_roi_paths_cpu.py does that without a GPU, and the GPU tests assert it again before they launch anything.

The kernels place sample i of a bin at fmaf(i, sub, start) (one rounding), oracle/nn.py at start + float32(i) * sub (two).  The
two can differ by one ulp; where that flips a sample's validity or moves it across a cell boundary, kernel and oracle compute
different (both defensible) operators.  `bin_paths` flags such samples; the tests require inputs without any, so that no
tolerance has to absorb them."""
import numpy as np

f32 = np.float32
K_WIN_MAX = 8            # kWinMax
K_BINS_MAX = 64          # kBinsMax (= kMfmaK)
CLASSES = ('none', '<=2', '3', '4', '5-8', '>8')


def _round_half_away(v):
    v = np.asarray(v, f32)
    return (np.floor(np.abs(v) + f32(0.5)) * np.sign(v)).astype(f32)


def bin_starts(rois, trans, P, S, scale, trans_std):
    """roi_geom in float32, every product and sum rounded on its own (the kernel compiles it with contraction off).
    -> wstart, hstart (R, P, P), sub_w, sub_h (R,)"""
    rois = np.asarray(rois, f32)
    R = rois.shape[0]
    scale, trans_std = f32(scale), f32(trans_std)
    sw = _round_half_away(rois[:, 1]) * scale - f32(0.5)
    sh = _round_half_away(rois[:, 2]) * scale - f32(0.5)
    ew = (_round_half_away(rois[:, 3]) + f32(1)) * scale - f32(0.5)
    eh = (_round_half_away(rois[:, 4]) + f32(1)) * scale - f32(0.5)
    rw, rh = np.maximum(ew - sw, f32(0.1)), np.maximum(eh - sh, f32(0.1))
    bw, bh = rw / f32(P), rh / f32(P)
    if trans is not None:
        t = np.asarray(trans, f32)
        tx, ty = t[:, 0] * trans_std, t[:, 1] * trans_std
    else:
        tx = ty = np.zeros((R, P, P), f32)
    idx = np.arange(P, dtype=f32)
    ws = idx[None, None, :] * bw[:, None, None] + sw[:, None, None] + tx * rw[:, None, None]
    hs = idx[None, :, None] * bh[:, None, None] + sh[:, None, None] + ty * rh[:, None, None]
    assert ws.dtype == f32 and hs.dtype == f32
    return ws, hs, bw / f32(S), bh / f32(S)


def _axis(start, sub, S, dim):
    """One axis of every bin.  start (R, P, P) float32, sub (R,) float32.
    -> n valid (kernel's form), n valid (oracle's form), lo, hi (cell range of the kernel's valid samples), ambiguous (R,P,P,S)"""
    i = np.arange(S)
    sub3 = sub[:, None, None, None]
    st = start[..., None]
    fused = (i.astype(np.float64) * sub3.astype(np.float64) + st.astype(np.float64)).astype(f32)      # fmaf(i, sub, start)
    split = (st + i.astype(f32) * sub3).astype(f32)                                                    # start + float32(i) * sub
    res = []
    for w in (fused, split):
        ok = ~((w < f32(-0.5)) | (w > f32(dim) - f32(0.5)))
        c = np.minimum(np.maximum(w, f32(0)), f32(dim) - f32(1))
        res.append((ok, np.floor(c).astype(np.int64), np.ceil(c).astype(np.int64), c))
    (ok_k, fl_k, ce_k, c_k), (ok_o, fl_o, ce_o, _) = res
    amb = (ok_k != ok_o) | (ok_k & ok_o & ((fl_k != fl_o) | (ce_k != ce_o)))
    n = ok_k.sum(-1)
    lo = np.where(n > 0, np.floor(np.where(ok_k, c_k, np.inf).min(-1, initial=np.inf, where=ok_k)), 0)
    hi = np.where(n > 0, np.ceil(np.where(ok_k, c_k, -np.inf).max(-1, initial=-np.inf, where=ok_k)), -1)
    lo = np.where(n > 0, lo, 0).astype(np.int64)
    hi = np.where(n > 0, hi, -1).astype(np.int64)
    return n, ok_o.sum(-1), lo, hi, amb


def bin_paths(rois, trans, P, S, scale, trans_std, H, W):
    """-> dict: nx, ny (R,P,P) cells per axis of the bin's window (0 where the bin has no valid sample), count (valid samples,
    the kernels' form), count_oracle (oracle/nn.py's form), cls (R,P,P) index into CLASSES, ambiguous (number of samples whose
    validity, floor or ceil depends on how the position was rounded), x_lo, x_hi, y_lo, y_hi."""
    ws, hs, sub_w, sub_h = bin_starts(rois, trans, P, S, scale, trans_std)
    nvx, nvx_o, x_lo, x_hi, amb_x = _axis(ws, sub_w, S, W)
    nvy, nvy_o, y_lo, y_hi, amb_y = _axis(hs, sub_h, S, H)
    count = nvx * nvy
    nx = np.where(count > 0, x_hi - x_lo + 1, 0)
    ny = np.where(count > 0, y_hi - y_lo + 1, 0)
    m = np.maximum(nx, ny)
    cls = np.select([count == 0, m <= 2, m == 3, m == 4, m <= K_WIN_MAX], [0, 1, 2, 3, 4], 5)
    return {'nx': nx, 'ny': ny, 'count': count, 'count_oracle': nvx_o * nvy_o, 'cls': cls,
            'ambiguous': int(amb_x.sum() + amb_y.sum()), 'x_lo': x_lo, 'x_hi': x_hi, 'y_lo': y_lo, 'y_hi': y_hi}


def class_counts(paths):
    return {name: int((paths['cls'] == k).sum()) for k, name in enumerate(CLASSES)}


# ---------------------------------------------------------------------------------------------
# The inputs of the GPU tests.  RoI recipe of tests/test_gpu_nn_ops.py::test_dpsroi_pool_fwd_bwd_vs_oracle (random centres and
# sizes, one RoI partly outside, one covering the whole map, one of one pixel) plus two RoIs wholly outside the map (upper left
# and right: no valid sample, with or without offsets) and, where a case is after large windows, one covering most of the map.
# ---------------------------------------------------------------------------------------------
SC = 16                  # pixels per map cell (spatial_scale = 1 / SC)
TRANS_STD = 0.1
OUTSIDE_ROWS = (3, 4)    # rows of the wholly-outside RoIs


def make_rois(rs, B, H, W, R, wh_max, big):
    rois = np.zeros((R, 5), f32)
    rois[:, 0] = rs.randint(0, B, R)
    c = rs.uniform(20, SC * min(H, W) - 20, (R, 2))
    wh = rs.uniform(4, wh_max, (R, 2))
    rois[:, 1:3], rois[:, 3:5] = c - wh / 2, c + wh / 2
    rois[0, 1:] = [-30, -20, 40, 50]                       # partly outside
    rois[1, 1:] = [0, 0, SC * W - 1, SC * H - 1]           # whole map
    rois[2, 1:] = [33, 47, 34, 48]                         # tiny: every sample of a bin in one cell
    rois[3, 1:] = [-260, -230, -90, -70]                   # wholly outside, upper left
    rois[4, 1:] = [SC * W + 80, 10, SC * W + 190, 90]      # wholly outside, to the right
    if big:
        rois[5, 1:] = [0.07 * SC * W, 0.05 * SC * H, 0.94 * SC * W, 0.93 * SC * H]      # most of the map
    return rois


class PoolCase(object):
    """One parametrised case: shapes, the window classes it must reach (with and without offsets) and its seed.
    G = 1: sn_dpsroi_pool_*, channels C; G > 1: sn_psroi_pool_*, D output channels on a map of D * G * G."""

    def __init__(self, name, B, C, H, W, R, P, S, reach, seed=3, wh_max=120.0, big=False, with_trans=True, G=1, dense=False):
        self.name, self.B, self.C, self.H, self.W, self.R, self.P, self.S = name, B, C, H, W, R, P, S
        self.reach, self.seed, self.wh_max, self.big, self.with_trans, self.G = reach, seed, wh_max, big, with_trans, G
        self.dense = dense      # one image whose whole-map RoI samples every cell: no untouched region (in one mode at least)

    def __repr__(self):
        return self.name

    @property
    def modes(self):
        return ((False, 0.0), (True, TRANS_STD)) if self.with_trans else ((False, 0.0),)

    def inputs(self):
        """-> rois (R,5), trans (R,2,P,P): a function of the case alone (the CPU test and the GPU test see the same arrays)"""
        rs = np.random.RandomState(self.seed)
        rois = make_rois(rs, self.B, self.H, self.W, self.R, self.wh_max, self.big)
        trans = (rs.standard_normal((self.R, 2, self.P, self.P)) * 0.5).astype(f32)
        return rois, trans

    @property
    def fast_oracle(self):
        """The loop statement of oracle/nn.py costs ~150 us per sample (forward + backward): beyond 2000 bins, or 16 000 samples, the
        sparse-operator form (pinned to the loops by tests/test_oracle_graph_cpu.py) keeps a case to seconds."""
        bins = self.R * self.P * self.P
        return bins > 2000 or bins * self.S * self.S > 16000

    def paths(self, with_trans):
        rois, trans = self.inputs()
        return bin_paths(rois, trans if with_trans else None, self.P, self.S, 1.0 / SC, TRANS_STD if with_trans else 0.0,
                         self.H, self.W)

    def check_reach(self):
        """The condition every test of this case states before it runs anything: no rounding-dependent sample, every class the
        case is there for non-empty, and the wholly-outside RoIs without a valid sample -- in each mode the case runs."""
        for with_trans, _ in self.modes:
            p = self.paths(with_trans)
            n = class_counts(p)
            assert p['ambiguous'] == 0, (self.name, with_trans, p['ambiguous'])
            assert np.array_equal(p['count'], p['count_oracle']), (self.name, with_trans)
            for c in self.reach:
                assert n[c] > 0, (self.name, with_trans, c, n)
            assert (p['count'][list(OUTSIDE_ROWS)] == 0).all(), (self.name, with_trans)
        return True


def untouched_cells(rois, trans, B, H, W, P, S, scale, trans_std):
    """(B, H, W) bool: map cells that carry no bilinear weight of any sample of any RoI (oracle/nn.py's sampling operator has an
    all-zero column there): the data gradient is exactly zero on them."""
    from oracle import nn as onn
    A = onn._dpsroi_operators(rois, trans, B, H, W, P, S, scale, trans_std)[0]
    return (np.asarray(abs(A).sum(0)).ravel() == 0).reshape(B, H, W)


ALL = CLASSES
SMALL = ('none', '<=2', '3', '4')

DPSROI_CASES = [
    # generic kernels (pooled * pooled > 64): dpsroi_fwd_kernel, dpsroi_bwd_data_kernel (dynamic LDS), dpsroi_bwd_trans_kernel (its
    # window walk is also the oversized branch of dpsroi_bwd_trans_roi_kernel: trans_window_walk)
    PoolCase('generic-P14-mask-head', 2, 64, 20, 24, 24, 14, 4, SMALL),
    PoolCase('generic-P14-large-map', 1, 64, 72, 80, 8, 14, 4, ('none', '<=2', '3', '4', '5-8'), wh_max=700.0, big=True, dense=True),
    PoolCase('generic-P16-S2', 1, 64, 12, 12, 8, 16, 2, ('none', '<=2', '3'), dense=True),
    # per-RoI kernels, every window class
    PoolCase('roi-P2-all-classes', 2, 64, 24, 20, 24, 2, 4, ALL),
    PoolCase('roi-P1', 2, 64, 24, 20, 16, 1, 4, ('none', '<=2', '5-8', '>8')),
    PoolCase('roi-P7-large-map', 1, 64, 72, 80, 12, 7, 4, ALL, wh_max=700.0, big=True),
    # sample_per_part > 4: the <kMaxS> instantiations; S = 1
    PoolCase('roi-S8', 2, 64, 14, 12, 24, 7, 8, SMALL),
    PoolCase('roi-S5', 2, 64, 14, 12, 24, 7, 5, SMALL),
    PoolCase('roi-P8-S8-large-map', 2, 64, 72, 80, 10, 8, 8, ALL, wh_max=700.0, big=True),
    PoolCase('roi-S1-C8', 1, 8, 9, 11, 12, 3, 1, ('none', '<=2')),
    # MFMA data gradient: 64 bins and two scan rounds, two channel chunks, channel masking
    PoolCase('mfma-P8-R300', 2, 128, 16, 20, 300, 8, 4, SMALL),
    PoolCase('mfma-C512', 2, 512, 10, 14, 40, 7, 4, ('none', '<=2', '3')),
    PoolCase('mfma-C24', 2, 24, 12, 12, 9, 7, 4, ('none', '<=2'), with_trans=False),
]

# position-sensitive kernels: (B, D, H, W, R, P = G, S)
PSROI_CASES = [
    PoolCase('ps-D40-S4', 1, 40, 40, 44, 12, 3, 4, ALL, wh_max=400.0, big=True, G=3),
    PoolCase('ps-D5-S8', 1, 5, 40, 44, 12, 3, 8, ALL, wh_max=400.0, big=True, G=3),
]


# ---------------------------------------------------------------------------------------------
# Deformable sampling: the candidate window of deform_col2im_data_mfma_kernel, restated
# ---------------------------------------------------------------------------------------------
def deform_out_size(H, W, KH, KW, stride, pad, dil):
    return (H + 2 * pad - dil * (KH - 1) - 1) // stride + 1, (W + 2 * pad - dil * (KW - 1) - 1) // stride + 1


def deform_candidate_range(t0, dim_out, dmax, KH, KW, stride, pad, dil):
    """Output rows (or columns) the pruned scan of the data gradient visits for the 4-cell tile at t0, from max |offset| = dmax:
    a sample at o * stride - pad + k * dil + offset touches cells floor(p) and floor(p) + 1, so o * stride lies in
    [t0 - 1 - dmax + pad - span * dil, t0 + 4 + dmax + pad); the kernel widens dmax to ceil(dmax) + 1.  -> (lo, hi) inclusive"""
    Di = int(np.ceil(dmax)) + 1
    span = max(KH, KW) - 1
    lo = max(0, -((-(t0 - Di + pad - span * dil)) // stride))
    hi = min(dim_out - 1, (t0 + 3 + Di + pad) // stride)
    return lo, hi


def deform_needed_range(t0, dim_out, offs_min, offs_max, k_max, stride, pad, dil):
    """Output rows (or columns) that CAN reach the tile at t0 with offsets in [offs_min, offs_max]: a lower bound every correct
    window contains"""
    need = [o for o in range(dim_out)
            if o * stride - pad + offs_max > t0 - 1 and o * stride - pad + k_max * dil + offs_min < t0 + 4]
    return (need[0], need[-1]) if need else (0, -1)
