"""-m gpu: every dispatch branch of csrc/roi_deform.hip against oracle/nn.py -- the generic D-PSRoI kernels (pooled * pooled > 64:
the mask head's 14 x 14 pool), the per-RoI kernels at every window class (unrolled 2 / 3 / 4 cells, the rolled 5 - 8 loop, the
oversized on-the-fly path), the <kMaxS> instantiations (sample_per_part > 4) and S = 1, the MFMA data gradient at 64 bins /
two channel chunks / a channel count that is no multiple of 64, the position-sensitive kernels with large windows, and the
deformable sampling kernels away from 3 x 3 / stride 1.  tests/test_gpu_nn_ops.py holds the same operators at P = 7, S = 4 on
small maps; the tolerances here are the ones stated there.

Every pooling case first shows ON THE CPU (tests/roi_paths_util.py) that its inputs reach the window classes it is there for
and hold no sample whose cell depends on how its position was rounded -- a condition, not a tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import roi_paths_util as rp  # noqa: E402
from gpu_util import assert_close, dev, f16r, from_nhwc, to_nhwc_f16  # noqa: E402
from oracle import nn as onn  # noqa: E402


def _hip():
    from sniper_amd import hip
    return hip


def _pool_case(case):
    """Forward, data gradient (fp32 and fp16) and offset gradient of one case, with and without offsets, against oracle/nn.py in
    float64 on fp16-rounded inputs; outputs poisoned with 7.0 (every element must be written); a second backward bit-equal to
    the first; rows of the wholly-outside RoIs exactly zero in out and d_trans; cells no RoI touches exactly zero in d_data.
    G > 1 (position-sensitive): the operator's channel order against the oracle, then the group-major order against the oracle
    and bit-equal to the first."""
    hip = _hip()
    assert case.check_reach()
    B, H, W, R, P, S, G, D = case.B, case.H, case.W, case.R, case.P, case.S, case.G, case.C
    C = D * G * G
    scale = 1.0 / rp.SC
    rois, trans = case.inputs()
    rs = np.random.RandomState(case.seed + 1000)
    data = rs.standard_normal((B, C, H, W)).astype(np.float32)
    dout = rs.standard_normal((R, D, P, P)).astype(np.float32)
    data64, dout64 = f16r(data).astype(np.float64), f16r(dout).astype(np.float64)
    fwd_o, bwd_o = (onn.dpsroi_pool_fast, onn.dpsroi_pool_backward_fast) if case.fast_oracle else (onn.dpsroi_pool, onn.dpsroi_pool_backward)
    dd = to_nhwc_f16(data)
    dod = torch.from_numpy(np.ascontiguousarray(dout.transpose(0, 2, 3, 1))).to(dev()).half()
    td = lambda z: None if z is None else torch.from_numpy(z).to(dev())
    ws = torch.empty(hip.query('sn_dpsroi_bwd_workspace_bytes', R), dtype=torch.uint8, device=dev())
    outside = list(rp.OUTSIDE_ROWS)
    perm = torch.from_numpy(np.array([d * G * G + g for g in range(G * G) for d in range(D)])).to(dev())

    def forward(map_d, tr, tstd, gm):
        out = torch.full((R, P, P, D), 7.0, dtype=torch.float16, device=dev())
        if G == 1:
            hip.call('sn_dpsroi_pool_fwd', map_d, td(rois), td(tr), out, R, H, W, C, P, S, scale, tstd, hip.stream())
        else:
            hip.call('sn_psroi_pool_fwd', map_d, td(rois), td(tr), out, R, H, W, D, G, P, S, scale, tstd, gm, hip.stream())
        return out

    def backward(map_d, tr, tstd, f32, gm):
        d_data = torch.full((B, H, W, C), 7.0, dtype=torch.float32 if f32 else torch.float16, device=dev())
        d_trans = torch.full((R, 2, P, P), 7.0, dtype=torch.float32, device=dev()) if tr is not None else None
        if G == 1:
            hip.call('sn_dpsroi_pool_bwd', dod, map_d, td(rois), td(tr), d_data, f32, d_trans, R, B, H, W, C, P, S, scale, tstd, ws,
                     hip.stream())
        else:
            hip.call('sn_psroi_pool_bwd', dod, map_d, td(rois), td(tr), d_data, f32, d_trans, R, B, H, W, D, G, P, S, scale, tstd, gm,
                     ws, hip.stream())
        return d_data, d_trans

    for with_trans, tstd in case.modes:
        tr = trans if with_trans else None
        what = '%s trans=%d' % (case.name, with_trans)
        want = fwd_o(data64, rois, tr, P, S, scale, tstd, group_size=G)
        wd, wtr = bwd_o(dout64, data64, rois, tr, P, S, scale, tstd, group_size=G)
        untouched = rp.untouched_cells(rois, tr, B, H, W, P, S, scale, tstd)
        assert untouched.any() or case.dense, what
        assert (want[outside] == 0).all() and (wd.transpose(0, 2, 3, 1)[untouched] == 0).all()
        untouched_d = torch.from_numpy(untouched).to(dev())
        layouts = ((0, dd),) if G == 1 else ((0, dd), (1, dd[..., perm].contiguous()))
        first = None
        for gm, map_d in layouts:
            unperm = (lambda t: t) if gm == 0 else (lambda t: t[..., torch.argsort(perm)])
            out = forward(map_d, tr, tstd, gm)
            assert_close(from_nhwc(out), want, 1e-2, 1e-2, 'fwd ' + what)
            assert (out[outside] == 0).all(), what
            runs = {}
            for f32 in (1, 0):
                d_data, d_trans = runs[f32] = backward(map_d, tr, tstd, f32, gm)
                tol = 1e-3 if f32 else 1e-2
                assert_close(from_nhwc(unperm(d_data)), wd, tol, tol * np.abs(wd).max(), 'd_data f32=%d %s' % (f32, what))
                assert (d_data[untouched_d] == 0).all(), what
                if tr is not None:
                    assert_close(d_trans.cpu().numpy(), wtr, 1e-3, 1e-3 * np.abs(wtr).max(), 'd_trans ' + what)
                    assert (d_trans[outside] == 0).all(), what
            # fixed summation order: a second call writes the same bits
            again = backward(map_d, tr, tstd, 0, gm)
            assert torch.equal(again[0], runs[0][0]), what
            if tr is not None:
                assert torch.equal(again[1], runs[0][1]) and torch.equal(runs[1][1], runs[0][1]), what
            if first is None:
                first = (out, runs[0][0], runs[0][1])
            else:
                # group-major map: the arithmetic per output and the entry order of the data gradient do not depend on the layout
                assert torch.equal(out, first[0]) and torch.equal(unperm(runs[0][0]), first[1]), what
                if tr is not None:
                    assert torch.equal(runs[0][1], first[2]), what


@pytest.mark.parametrize('case', rp.DPSROI_CASES, ids=repr)
def test_dpsroi_pool_paths_vs_oracle(case):
    """sn_dpsroi_pool_fwd / _bwd (group_size 1).  generic-*: dpsroi_fwd_kernel, dpsroi_bwd_data_kernel, dpsroi_bwd_trans_kernel
    (pooled 14: the mask head; 16: the largest the backward accepts; the 72 x 80 map: 5 - 8 cell windows).  roi-*: the per-RoI
    kernels at every window class, <kMaxS> at S = 8 and S = 5 with and without oversized windows, S = 1 with C / 8 = 1.  mfma-*:
    64 bins with 300 RoIs (two scan rounds, several flushes, all 64 lanes of phase A), C = 512 (two channel chunks), C = 24
    (masked channels of the MFMA operand and of the store; without offsets: the offset gradient needs C / 8 a power of two)."""
    _pool_case(case)


@pytest.mark.parametrize('case', rp.PSROI_CASES, ids=repr)
def test_position_sensitive_pool_paths_vs_oracle(case):
    """sn_psroi_pool_fwd / _bwd (G = P = 3) on a 40 x 44 map with RoIs of most of the map: the sample-loop branch of
    psroi_ps_bwd_trans_kernel (windows beyond 8 cells), the wave-per-bin forward (D = 40 >= 32) and the thread-per-element one
    (D = 5) with large windows, S = 8; both channel orders (psroi_ps_bwd_data_kernel<false> / <true>: one template, built from
    the RoI scan and bin weights the dpsroi_bwd_data kernels use)."""
    _pool_case(case)


# ---------------------------------------------------------------------------------------------
# Deformable sampling away from 3 x 3, stride 1, pad = dil
# ---------------------------------------------------------------------------------------------
# name, C, DG, KH, KW, stride, pad, dil, H, W, offset gradient?
DEFORM_CASES = [
    ('s2-3x3-p1', 64, 4, 3, 3, 2, 1, 1, 14, 12, True),
    ('s2-3x3-p2-d2', 128, 1, 3, 3, 2, 2, 2, 13, 12, True),
    ('s1-1x1', 64, 4, 1, 1, 1, 0, 1, 14, 12, True),
    ('s1-1x3', 64, 2, 1, 3, 1, 1, 1, 12, 14, True),
    ('s2-cg8', 32, 4, 3, 3, 2, 1, 1, 14, 12, True),
    ('s2-cg24', 96, 4, 3, 3, 2, 1, 1, 14, 12, False),       # cg / 8 = 3 is no power of two: data gradient only
    ('s2-two-slabs', 512, 1, 3, 3, 2, 1, 1, 12, 14, True),
]
DEFORM_N = 2


def _deform_offsets(rs, kind, DG, KH, KW, stride, pad, dil, H, W):
    """Offsets (N, 2*T*DG, Ho, Wo), every value exact in fp16 (one oracle serves the fp32- and the fp16-offset launch).
    'far': ~1.5 cells with one sampling point 40 cells outside (the window opens completely); 'few': |offset| <= 1.5 or 2.5 cells;
    'sub': |offset| <= 0.75 of a cell.  'few' and 'sub' carry |offset| = dmax exactly, placed where the pruned scan's window
    ends: on the last candidate row / column of a tile pointing back into it, on the first pointing forward into it -- a window
    one row short drops them.  -> offsets, dmax, number of samples planted on a window's last row / column"""
    T = KH * KW
    Ho, Wo = rp.deform_out_size(H, W, KH, KW, stride, pad, dil)
    off = rs.standard_normal((DEFORM_N, 2 * T * DG, Ho, Wo))
    if kind == 'far':
        off = f16r(off * 1.5).astype(np.float64)
        off[0, :, 0, 0] = 40.0
        return off.astype(np.float32), 40.0, 0
    # (the last candidate row of a tile is (t0 + 3 + Di + pad) // stride, Di = ceil(dmax) + 1; at stride 2 a sample on it reaches back
    # into the tile only where t0 + 2 + Di + pad is even: a maximum of 1.5 cells for an odd pad, 2.5 for an even one)
    few = 1.5 if (stride == 2 and pad % 2 == 1) else 2.5
    dmax = few if kind == 'few' else 0.75
    off = f16r(np.clip(off * (1.0 if kind == 'few' else 0.3), -dmax, dmax)).astype(np.float64)
    planted, used = 0, set()
    for comp, (dim, dim_out, K) in enumerate(((H, Ho, KH), (W, Wo, KW))):
        other_out, other_dim = (Wo, W) if comp == 0 else (Ho, H)
        # a position on the other axis that is inside the map with a zero offset at tap 0 / at the last tap
        for t0 in range(0, dim, 4):
            lo, hi = rp.deform_candidate_range(t0, dim_out, dmax, KH, KW, stride, pad, dil)
            for o, k, sign in ((hi, 0, -1.0), (lo, K - 1, 1.0)):
                p = o * stride - pad + k * dil + sign * dmax
                reaches = (t0 + 3 <= p < t0 + 4) if sign < 0 else (t0 - 1 < p < t0)
                if not (reaches and 0 <= p < dim):
                    continue
                tap = k * KW if comp == 0 else k           # (kh = k, kw = 0) or (kh = 0, kw = k)
                oo = [q for q in range(other_out) if 0 <= q * stride - pad < other_dim]
                if not oo:
                    continue
                q = oo[len(oo) // 2]
                idx = (o, q) if comp == 0 else (q, o)
                if (idx, tap) in used:
                    continue
                used.add((idx, tap))
                for n in range(DEFORM_N):
                    for g in range(DG):
                        off[n, g * 2 * T + 2 * tap + comp, idx[0], idx[1]] = sign * dmax
                        off[n, g * 2 * T + 2 * tap + 1 - comp, idx[0], idx[1]] = 0.0
                planted += 1 if sign < 0 else 0
    if float(np.abs(off).max()) < dmax:
        off[1, 2 * T - 1, Ho - 1, Wo - 1] = dmax
    assert np.array_equal(f16r(off), off) and float(np.abs(off).max()) == dmax
    return off.astype(np.float32), dmax, planted


@pytest.mark.parametrize('name,C,DG,KH,KW,stride,pad,dil,H,W,with_doff', DEFORM_CASES, ids=[c[0] for c in DEFORM_CASES])
def test_deformable_sampling_strides_and_kernel_shapes_vs_oracle(name, C, DG, KH, KW, stride, pad, dil, H, W, with_doff):
    """sn_deform_im2col / sn_deform_col2im against onn.deform_im2col / deform_col2im: stride 2 (the candidate window of the data
    gradient divides by the stride), pad != dil, span 0 (1 x 1), KH != KW, cg = 8 / 24 (a 64-thread workgroup with masked
    channels; cg / 8 = 3 has no offset gradient), cg = 512 (two slabs).  fp32 and fp16 offsets, fp32 and fp16 data gradient.
    With and without the max |offset| workspace the data gradient is bit-equal, and for sub-cell offsets the window it implies
    (restated on the CPU from the workspace's value) really is smaller than the full scan."""
    hip = _hip()
    N, T, oc = DEFORM_N, KH * KW, 2 * KH * KW * DG
    Ho, Wo = rp.deform_out_size(H, W, KH, KW, stride, pad, dil)
    rs = np.random.RandomState(len(name) * 131 + C)
    data = rs.standard_normal((N, C, H, W)).astype(np.float32)
    dcol = rs.standard_normal((N, Ho, Wo, T, C)).astype(np.float32)
    dd, dcd = to_nhwc_f16(data), torch.from_numpy(dcol).to(dev()).half()
    data64, dcol64 = f16r(data).astype(np.float64), f16r(dcol).astype(np.float64)
    planted_last = 0
    for kind in ('far', 'few', 'sub'):
        off, dmax, planted = _deform_offsets(rs, kind, DG, KH, KW, stride, pad, dil, H, W)
        planted_last += planted
        # the window the kernel derives from max |offset|, tile by tile
        cand = sum((lambda y, x: max(y[1] - y[0] + 1, 0) * max(x[1] - x[0] + 1, 0))(
            rp.deform_candidate_range(y0, Ho, dmax, KH, KW, stride, pad, dil), rp.deform_candidate_range(x0, Wo, dmax, KH, KW, stride, pad, dil))
            for y0 in range(0, H, 4) for x0 in range(0, W, 4))
        tiles = len(range(0, H, 4)) * len(range(0, W, 4))
        if kind == 'sub':
            assert cand < tiles * Ho * Wo, (name, cand, tiles * Ho * Wo)
        else:
            assert kind != 'far' or cand == tiles * Ho * Wo
        want_col = onn.deform_im2col(data64, off.astype(np.float64), KH, KW, stride, pad, dil, DG)
        want_dd, want_do = onn.deform_col2im(dcol64, data64, off.astype(np.float64), KH, KW, stride, pad, dil, DG)
        assert np.abs(want_dd).max() > 0
        off_nhwc = torch.from_numpy(np.ascontiguousarray(off.transpose(0, 2, 3, 1))).to(dev())
        for odt, offd in ((1, off_nhwc), (0, off_nhwc.half())):
            what = '%s %s offsets fp%d' % (name, kind, 32 if odt else 16)
            col = torch.full((N * Ho * Wo, T, C), 7.0, dtype=torch.float16, device=dev())
            hip.call('sn_deform_im2col', dd, offd, col, N, H, W, C, KH, KW, stride, pad, dil, DG, oc, odt, hip.stream())
            assert_close(col.float().cpu().numpy().reshape(want_col.shape), want_col, 1e-2, 1e-2, 'im2col ' + what)
            for f32 in (1, 0):
                full = torch.full((N, H, W, C), 7.0, dtype=torch.float32 if f32 else torch.float16, device=dev())
                d_off = torch.full((N, Ho, Wo, oc), 7.0, dtype=offd.dtype, device=dev()) if with_doff else None
                hip.call('sn_deform_col2im', dcd, dd, offd, full, f32, d_off, N, H, W, C, KH, KW, stride, pad, dil, DG, oc, odt, None,
                         hip.stream())
                pruned = torch.full_like(full, 7.0)
                wsd = torch.full((16,), 0x55, dtype=torch.uint8, device=dev())
                hip.call('sn_deform_col2im', dcd, dd, offd, pruned, f32, None, N, H, W, C, KH, KW, stride, pad, dil, DG, oc, odt, wsd,
                         hip.stream())
                assert wsd[:4].view(torch.float32).item() == dmax, what
                assert torch.equal(pruned, full), what
                tol = 1e-3 if f32 else 1e-2
                assert_close(from_nhwc(full), want_dd, tol, tol * np.abs(want_dd).max(), 'd_data f32=%d %s' % (f32, what))
                if with_doff:
                    # (an fp16 d_offset rounds to 2^-11 relative: inside the same bound)
                    assert_close(d_off.float().cpu().numpy().transpose(0, 3, 1, 2), want_do, 1e-3, 1e-3 * np.abs(want_do).max(),
                                 'd_offset ' + what)
    if stride == 2:
        assert planted_last > 0, name      # a sample on the last candidate row / column of a tile, reaching back into it
