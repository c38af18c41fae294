"""-m gpu: grouped deformable convolution (csrc/gdeform.hip) -- the three kernels in exact arithmetic against the float64 oracle
(oracle.nn.deform_im2col / deform_col2im; the per-group contraction is written here), the forward pass at zero offsets against
sn_gconv_fwd bit for bit, the lowered step on random data, hipGraph replay and dense-twin gradient parity of a small graph, and
three optimizer steps of the resnext101_e2e_dcn preset."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import assert_close, dev, f16r, from_nhwc, to_nhwc_f16, w_to_otI  # noqa: E402

T = 9
# (N, H, W, stride, pad, dil): a 16-pixel tile tail and a 32-pixel chunk tail (143 pixels); whole tiles; stride 2
CASES = {'a': (1, 13, 11, 1, 2, 2), 'b': (2, 8, 8, 1, 2, 2), 'c': (1, 13, 11, 2, 1, 1)}
# (C, groups, DG): Cg = 4 / one slab;  Cg = 32 (NB = 2), a deformable-group boundary between two slabs;  Cg = 16, three slabs
# (one wave per workgroup);  Cg = 8, four slabs, two per deformable group
COMBOS = [(32, 8, 1), (64, 2, 2), (96, 6, 3), (128, 16, 2)]


def _hip():
    from sniper_amd import hip
    return hip


def _out(H, k, s, p, d):
    return (H + 2 * p - d * (k - 1) - 1) // s + 1


def _plant(off, rs, H, W, stride, pad, dil, DG, values):
    """Put samples at chosen coordinates: for every v in `values` (a function of the extent), a few (n, group, tap, oy, ox) get
    the offset that makes the y (and, at another place, the x) coordinate exactly v(dim)."""
    N, _, Ho, Wo = off.shape
    for v in values:
        for axis in (0, 1):
            for _ in range(3):
                n, g, t, oy, ox = rs.randint(N), rs.randint(DG), rs.randint(T), rs.randint(Ho), rs.randint(Wo)
                kh, kw = divmod(t, 3)
                base = (oy * stride - pad + kh * dil) if axis == 0 else (ox * stride - pad + kw * dil)
                off[n, g * 2 * T + 2 * t + axis, oy, ox] = v(H if axis == 0 else W) - base
    return off


_EXACT_PLANTS = [lambda d: d - 1.0, lambda d: -0.5, lambda d: d - 0.5, lambda d: float(d), lambda d: 0.0, lambda d: d - 1.5]


def _reference(x, off, w, dy, groups, DG, stride, pad, dil):
    """float64: y (M, O), dcol (M, T, C), dw (O, Cg, 3, 3) of the grouped deformable convolution; the sampled column from the oracle,
    the per-group contraction here"""
    from oracle import nn as onn
    N, C = x.shape[:2]
    O, Cg = w.shape[:2]
    Og = O // groups
    col = onn.deform_im2col(x.astype(np.float64), off.astype(np.float64), 3, 3, stride, pad, dil, DG)        # (N, Ho, Wo, T, C)
    M = col.shape[0] * col.shape[1] * col.shape[2]
    colg = col.reshape(M, T, groups, Cg)
    wg = w.astype(np.float64).reshape(groups, Og, Cg, T)
    y = np.einsum('mtgc,goct->mgo', colg, wg).reshape(M, O)
    dyg = dy.astype(np.float64).transpose(0, 2, 3, 1).reshape(M, groups, Og)
    dcol = np.einsum('mgo,goct->mtgc', dyg, wg).reshape(M, T, C)
    dw = np.einsum('mgo,mtgc->goct', dyg, colg).reshape(O, Cg, 3, 3)
    return y, dcol, dw


def _launch_all(x, off, w, dy, groups, DG, stride, pad, dil, extra=0, off_f32=False):
    """sn_gdeform_fwd / _dcol / _wgrad (twice: the same bits) on device copies -> y (M, O), dcol (M, T, C), dw (O, T, Cg) as numpy"""
    hip = _hip()
    N, C, H, W = x.shape
    O, Cg = w.shape[:2]
    Ho, Wo = _out(H, 3, stride, pad, dil), _out(W, 3, stride, pad, dil)
    M = N * Ho * Wo
    xps, yps, ops = C + extra, O + extra, off.shape[1] + (8 if extra else 0)
    xd = torch.full((N, H, W, xps), 7.0, dtype=torch.float16, device=dev())
    xd[..., :C] = to_nhwc_f16(x)
    od = torch.full((N, Ho, Wo, ops), 3.0, dtype=torch.float32 if off_f32 else torch.float16, device=dev())
    od[..., :off.shape[1]] = torch.from_numpy(np.ascontiguousarray(off.transpose(0, 2, 3, 1))).to(dev()).to(od.dtype)
    wd = torch.from_numpy(w_to_otI(w)).to(dev()).half().contiguous()
    dyd = torch.full((N, Ho, Wo, yps), 5.0, dtype=torch.float16, device=dev())
    dyd[..., :O] = to_nhwc_f16(dy)
    odt = 1 if off_f32 else 0
    yd = torch.full((N, Ho, Wo, yps), 7.0, dtype=torch.float16, device=dev())
    hip.call('sn_gdeform_fwd', xd, od, wd, None, yd, N, H, W, C, xps, O, yps, groups, DG, 3, 3, stride, pad, dil, ops, odt, 0, hip.stream())
    if extra:
        assert float((yd[..., O:].float() - 7.0).abs().max()) == 0.0, 'the padding of the output pitch was written'
    dcol = torch.full((M, T, C), 9.0, dtype=torch.float16, device=dev())
    hip.call('sn_gdeform_dcol', dyd, wd, dcol, N, H, W, C, O, yps, groups, 3, 3, stride, pad, dil, hip.stream())
    need = hip.query('sn_gdeform_wgrad_workspace_bytes', N, H, W, C, O, groups, 3, 3, stride, pad, dil)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    runs = []
    for _ in range(2):
        dw = torch.zeros((O, T, Cg), dtype=torch.float32, device=dev())
        hip.call('sn_gdeform_wgrad', dyd, xd, od, dw, N, H, W, C, O, yps, xps, groups, DG, 3, 3, stride, pad, dil, ops, odt, ws, need,
                 hip.stream())
        runs.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(runs[0], runs[1]), 'weight gradient: not the same bits on a second run'
    return yd[..., :O].float().cpu().numpy().reshape(M, O), dcol.float().cpu().numpy(), runs[0].cpu().numpy()


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('C,groups,DG', COMBOS)
def test_exact_arithmetic(case, C, groups, DG):
    """data, weights and dy in {-1, 0, 1}, offsets multiples of 0.5 (bilinear weights in {0, 1/4, 1/2, 1}): |y| <= 288 in multiples of
    1/4 is exact in fp16, |dcol| <= 32, |dw| <= M in multiples of 1/4 is exact in fp32 in any order -- every element of the three
    kernels' outputs EQUALS the float64 reference.  Planted samples: on row H-1 / column W-1, at -0.5, H - 0.5, H, 0 and H - 1.5.
    Pixel pitches larger than C and O in (a, Cg = 32); fp32 offsets in (b, Cg = 8)."""
    N, H, W, stride, pad, dil = CASES[case]
    Cg = C // groups
    rs = np.random.RandomState(C + 3 * stride + H)
    Ho, Wo = _out(H, 3, stride, pad, dil), _out(W, 3, stride, pad, dil)
    x = rs.randint(-1, 2, (N, C, H, W)).astype(np.float32)
    off = rs.randint(-6, 7, (N, 2 * T * DG, Ho, Wo)).astype(np.float32) * 0.5
    off = _plant(off, rs, H, W, stride, pad, dil, DG, _EXACT_PLANTS)
    w = rs.randint(-1, 2, (C, Cg, 3, 3)).astype(np.float32)
    dy = rs.randint(-1, 2, (N, C, Ho, Wo)).astype(np.float32)
    assert np.array_equal(off, f16r(off)) and np.abs(off).max() <= 32 and np.array_equal(off * 2, np.rint(off * 2))
    want_y, want_dcol, want_dw = _reference(x, off, w, dy, groups, DG, stride, pad, dil)
    # the reference survives the formats the kernels write: a mismatch below is the kernel's
    assert np.array_equal(want_y.astype(np.float16).astype(np.float64), want_y) and np.abs(want_y).max() <= 288
    assert np.array_equal(want_dcol.astype(np.float16).astype(np.float64), want_dcol) and np.abs(want_dcol).max() <= 32
    assert np.array_equal(want_dw.astype(np.float32).astype(np.float64), want_dw) and np.abs(want_dw).max() <= N * Ho * Wo
    assert np.abs(want_y).max() > 4 and np.abs(want_dw).max() > 2          # (not a comparison of zeros)
    y, dcol, dw = _launch_all(x, off, w, dy, groups, DG, stride, pad, dil, extra=24 if (case, Cg) == ('a', 32) else 0,
                              off_f32=(case, Cg) == ('b', 8))
    assert np.array_equal(y.astype(np.float64), want_y), 'forward: %d of %d elements differ' % ((y != want_y).sum(), y.size)
    assert np.array_equal(dcol.astype(np.float64), want_dcol), 'dcol: %d of %d elements differ' % ((dcol != want_dcol).sum(), dcol.size)
    want_dw = w_to_otI(want_dw)
    assert np.array_equal(dw.astype(np.float64), want_dw), 'dw: %d of %d elements differ' % ((dw != want_dw).sum(), dw.size)


@pytest.mark.parametrize('case,C,groups,DG', [('a', 32, 8, 1), ('a', 64, 2, 2), ('c', 96, 6, 3), ('b', 128, 16, 2)])
def test_zero_offsets_equal_the_grouped_convolution_bit_for_bit(case, C, groups, DG):
    """every blend is 1 * v: sn_gdeform_fwd == sn_gconv_fwd on the same geometry and weights, random fp16 data, with bias and ReLU"""
    hip = _hip()
    N, H, W, stride, pad, dil = CASES[case]
    rs = np.random.RandomState(C + H)
    Ho, Wo = _out(H, 3, stride, pad, dil), _out(W, 3, stride, pad, dil)
    xd = to_nhwc_f16(rs.standard_normal((N, C, H, W)))
    wd = torch.from_numpy(w_to_otI(rs.standard_normal((C, C // groups, 3, 3)) / 8)).to(dev()).half().contiguous()
    bd = torch.from_numpy(rs.standard_normal(C).astype(np.float32)).to(dev())
    od = torch.zeros((N, Ho, Wo, 2 * T * DG), dtype=torch.float16, device=dev())
    for bias, relu in ((None, 0), (bd, 1)):
        ya = torch.empty((N, Ho, Wo, C), dtype=torch.float16, device=dev())
        yb = torch.empty_like(ya)
        hip.call('sn_gdeform_fwd', xd, od, wd, bias, ya, N, H, W, C, C, C, C, groups, DG, 3, 3, stride, pad, dil, 2 * T * DG, 0, relu,
                 hip.stream())
        hip.call('sn_gconv_fwd', xd, wd, bias, yb, N, H, W, C, C, C, C, groups, 3, 3, stride, pad, dil, relu, 0, hip.stream())
        torch.cuda.synchronize()
        assert torch.isfinite(ya).all() and float(ya.float().abs().max()) > 0.5
        assert torch.equal(ya.view(torch.int16), yb.view(torch.int16)), 'relu %d' % relu


def _gd_symbol(mx, C, groups, DG, head):
    data, offset = mx.sym.Variable('data'), mx.sym.Variable('offset')
    y = mx.contrib.sym.DeformableConvolution(data=data, offset=offset, name='res5a_conv2', num_filter=C, kernel=(3, 3), stride=(1, 1),
                                             pad=(2, 2), dilate=(2, 2), num_deformable_group=DG, num_group=groups, no_bias=True)
    return mx.sym.MakeLoss(data=y * mx.sym.Variable('head'), name='loss') if head else y


@pytest.mark.parametrize('N,H,W,C,groups,DG', [(1, 13, 11, 64, 2, 2), (2, 8, 8, 128, 16, 2)])
def test_grouped_deformable_convolution_lowered_vs_float64(N, H, W, C, groups, DG):
    """DeformableConvolutionStep with num_group > 1 as a whole -- sn_gdeform_fwd, sn_gdeform_wgrad through the executor's scratch,
    sn_gdeform_dcol -> sn_deform_col2im with the max-|offset| workspace -- against float64, with the dense step's test's tolerances
    (test_gpu_engine.py::test_deformable_convolution_lowered_vs_float64); training and test time.  Offsets: a few pixels at random,
    some exactly on cells, and planted samples on the last row / column, at -0.5, H - 0.5, H and +-1e4."""
    import sniper_amd.mx as mx
    from oracle import nn as onn
    from sniper_amd.engine.executor import Executor
    O, Cg = C, C // groups
    rs = np.random.RandomState(N * H + W + C)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    off = f16r(rs.standard_normal((N, 2 * T * DG, H, W)) * 1.5)
    off[:, ::5] = np.rint(off[:, ::5])
    off = f16r(_plant(off, rs, H, W, 1, 2, 2, DG, [lambda d: d - 1.0, lambda d: -0.5, lambda d: d - 0.5, lambda d: float(d),
                                                    lambda d: 1.0e4, lambda d: -1.0e4]))
    assert np.isfinite(off).all() and np.abs(off).max() > 9.0e3
    w = (rs.standard_normal((O, Cg, 3, 3)) / np.sqrt(Cg * T)).astype(np.float32)
    head = rs.standard_normal((N, O, H, W)).astype(np.float32)
    x64, w64, dy = f16r(x), f16r(w), f16r(head)
    want_y, want_dcol, want_dw = _reference(x64, off, w64, dy, groups, DG, 1, 2, 2)
    want_y = want_y.reshape(N, H, W, O).transpose(0, 3, 1, 2)
    want_dx, want_doff = onn.deform_col2im(want_dcol.reshape(N, H, W, T, C), x64.astype(np.float64), off.astype(np.float64), 3, 3, 1, 2, 2, DG)

    shapes = dict(data=(N, C, H, W), offset=(N, 2 * T * DG, H, W), head=(N, O, H, W))
    ex = Executor(_gd_symbol(mx, C, groups, DG, True), shapes, True)
    ex.set_params({'res5a_conv2_weight': w}, {})
    for node in ex.nodes:                      # the data and the offset field are produced by layers that need their gradients
        if node.op is None and node.name in ('data', 'offset'):
            ex.vals[(id(node), 0)].needs_grad = True
    step = [s for s in ex.steps if type(s).__name__ == 'DeformableConvolutionStep'][0]
    assert step.groups == groups and step.col is None and step.wT_flat is None
    got, add_grad = {}, ex.add_grad

    def spy(v, g, fmt):
        if v.name in ('data', 'offset'):
            got[v.name] = (g.clone(), fmt)
        return add_grad(v, g, fmt)
    ex.add_grad = spy
    ex.forward(dict(data=x, offset=off, head=head), is_train=True)
    y = step.y.t.clone()
    ex.backward()
    torch.cuda.synchronize()
    assert_close(from_nhwc(y), want_y, 1e-2, 1e-2 * np.abs(want_y).max(), 'gdcn train output')
    assert got['data'][1] == 'act' and got['offset'][1] == 'act'
    assert_close(from_nhwc(got['data'][0]), want_dx, 1e-2, 1e-2 * np.abs(want_dx).max(), 'gdcn d_data')
    assert_close(from_nhwc(got['offset'][0]), want_doff, 1e-2, 1e-2 * np.abs(want_doff).max(), 'gdcn d_offset')
    p = ex.params['res5a_conv2_weight']
    dw = p.to_reference(p.grad.detach().cpu().numpy())
    assert dw.shape == (O, Cg, 3, 3)
    assert_close(dw, want_dw, 1e-2, 1e-2 * np.abs(want_dw).max(), 'gdcn d_weight')

    ex_i = Executor(_gd_symbol(mx, C, groups, DG, False), dict(data=shapes['data'], offset=shapes['offset']), False)
    ex_i.set_params({'res5a_conv2_weight': w}, {})
    out = ex_i.forward(dict(data=x, offset=off), is_train=False)[0]
    torch.cuda.synchronize()
    assert_close(out.cpu().numpy(), want_y, 1e-2, 1e-2 * np.abs(want_y).max(), 'gdcn inference output')


# ---------------------------------------------------------------------------------------------------------------------------------
# a small graph: replay and the dense twin
# ---------------------------------------------------------------------------------------------------------------------------------
_G, _DG, _MID = 8, 2, 64          # the stage-4 unit of the mini graph: 64 channels in 8 groups of 8, two deformable groups


def _mini_graph(mx, groups, A=3):
    """frozen stem -> one ResNeXt unit (grouped 3x3, stride 2, projection shortcut) -> one stage-4 unit of resnext_mx_101_e2e_dcn
    (learned offsets, grouped deformable 3x3 with Cg = 8, identity shortcut) -> RPN head -> SoftmaxOutput + smooth-L1 MakeLoss.
    groups = 1: the dense twin (the same graph, a dense deformable convolution)."""
    data = mx.sym.Variable('data')
    label, target, weight = mx.sym.Variable('label'), mx.sym.Variable('bbox_target'), mx.sym.Variable('bbox_weight')
    x = mx.sym.BatchNorm(data=data, name='bn_data', fix_gamma=True, eps=2e-5, use_global_stats=True)
    x = mx.sym.Convolution(data=x, name='conv0', num_filter=64, kernel=(7, 7), stride=(2, 2), pad=(3, 3), no_bias=True)
    x = mx.sym.Cast(data=x, dtype=np.float16)
    x = mx.sym.BatchNorm(data=x, name='bn0', fix_gamma=False, eps=2e-5, use_global_stats=True)
    x = mx.sym.Activation(data=x, act_type='relu', name='relu0')
    x = mx.sym.Pooling(data=x, kernel=(3, 3), stride=(2, 2), pad=(1, 1), pool_type='max')

    def bn(x, name, relu=True):
        y = mx.sym.BatchNorm(data=x, name=name, fix_gamma=False, eps=2e-5, momentum=0.9)
        return mx.sym.Activation(data=y, act_type='relu', name=name + '_relu') if relu else y

    def conv(x, name, nf, stride=1):
        return mx.sym.Convolution(data=x, name=name, num_filter=nf, kernel=(1, 1), stride=(stride, stride), no_bias=True)

    n1 = 'stage3_unit1'
    c2 = mx.sym.Convolution(data=bn(conv(x, n1 + '_conv1', 64), n1 + '_bn1'), name=n1 + '_conv2', num_filter=64, num_group=8,
                            kernel=(3, 3), stride=(2, 2), pad=(1, 1), no_bias=True)
    b3 = bn(conv(bn(c2, n1 + '_bn2'), n1 + '_conv3', 128), n1 + '_bn3', relu=False)
    u1 = mx.sym.Activation(data=b3 + bn(conv(x, n1 + '_sc', 128, 2), n1 + '_sc_bn', relu=False), act_type='relu', name=n1 + '_relu')

    n2 = 'stage4_unit1'
    a1 = bn(conv(u1, n2 + '_conv1', _MID), n2 + '_bn1')
    off = mx.sym.Convolution(data=a1, name=n2 + '_offset', num_filter=2 * T * _DG, kernel=(3, 3), stride=(1, 1), pad=(2, 2),
                             dilate=(2, 2), cudnn_off=True)
    d2 = mx.contrib.sym.DeformableConvolution(data=a1, offset=off, name=n2 + '_conv2', num_filter=_MID, kernel=(3, 3), stride=(1, 1),
                                              pad=(2, 2), dilate=(2, 2), num_group=groups, num_deformable_group=_DG, no_bias=True)
    b3 = bn(conv(bn(d2, n2 + '_bn2'), n2 + '_conv3', 128), n2 + '_bn3', relu=False)
    u2 = mx.sym.Activation(data=b3 + u1, act_type='relu', name=n2 + '_relu')

    cat = mx.sym.Cast(data=mx.sym.Concat(u1, u2, name='cat4'), dtype=np.float32)
    r = mx.sym.Activation(data=mx.sym.Convolution(data=cat, kernel=(3, 3), pad=(1, 1), num_filter=64, name='rpn_conv_3x3'),
                          act_type='relu', name='rpn_relu')
    cls = mx.sym.Convolution(data=r, kernel=(1, 1), num_filter=2 * A, name='rpn_cls_score')
    box = mx.sym.Convolution(data=r, kernel=(1, 1), num_filter=4 * A, name='rpn_bbox_pred')
    cls_r = mx.sym.Reshape(data=cls, shape=(0, 2, -1, 0), name='rpn_cls_score_reshape')
    prob = mx.sym.SoftmaxOutput(data=cls_r, label=label, multi_output=True, normalization='valid', use_ignore=True,
                                ignore_label=-1, name='rpn_cls_prob', grad_scale=100.0)
    l1 = weight * mx.sym.smooth_l1(name='rpn_bbox_loss_', scalar=1.0, data=(box - target))
    loss = mx.sym.MakeLoss(name='rpn_bbox_loss', data=l1, grad_scale=3 * 100.0 / 64.0)
    return mx.sym.Group([prob, loss])


_A, _B, _S = 3, 2, 64
_F = _S // 8
_SHAPES = dict(data=(_B, 3, _S, _S), label=(_B, _A * _F * _F), bbox_target=(_B, 4 * _A, _F, _F), bbox_weight=(_B, 4 * _A, _F, _F))
_DW = 'stage4_unit1_conv2_weight'


@pytest.fixture(scope='module')
def mini():
    """parameters (reference layouts, matrices fp16-representable) and five feeds of the mini graph, made once"""
    import sniper_amd.mx as mx
    rs = np.random.RandomState(6)
    sym = _mini_graph(mx, _G, _A)
    args, _, auxs = sym.infer_shape(**_SHAPES)
    P, AUX = {}, {}
    for name, shp in zip(sym.list_arguments(), args):
        if name in _SHAPES:
            continue
        if name.endswith('_gamma'):
            P[name] = rs.uniform(0.5, 1.5, shp).astype(np.float32)
        elif '_offset_weight' in name:
            P[name] = f16r(rs.standard_normal(shp) * 0.02)              # offsets of a few tenths of a pixel
        else:
            v = (rs.standard_normal(shp) * (0.1 if len(shp) == 1 else np.sqrt(2.0 / np.prod(shp[1:])))).astype(np.float32)
            P[name] = f16r(v) if len(shp) > 1 else v
    for name, shp in zip(sym.list_auxiliary_states(), auxs):
        AUX[name] = rs.uniform(0.5, 1.5, shp).astype(np.float32)
    assert P[_DW].shape == (_MID, _MID // _G, 3, 3)
    feeds = [dict(data=f16r(rs.standard_normal((_B, 3, _S, _S)) * 2),
                  label=rs.choice([-1, 0, 1], size=(_B, _A * _F * _F), p=[0.5, 0.3, 0.2]).astype(np.float32),
                  bbox_target=rs.standard_normal((_B, 4 * _A, _F, _F)).astype(np.float32),
                  bbox_weight=(rs.uniform(size=(_B, 4 * _A, _F, _F)) < 0.2).astype(np.float32)) for _ in range(5)]
    return P, AUX, feeds


def _fixed(sym):
    return [n for n in sym.list_arguments() if any(p in n for p in ('conv0', 'bn0', 'bn_data'))]


def test_grouped_deformable_graph_replay_is_bit_equal_to_eager(monkeypatch, mini):
    """five steps eagerly and five with the captured forward+backward / optimizer graphs: every launch of gdeform.hip is
    deterministic and takes its scratch from the executor, so the outputs and the updated parameters are the same bits"""
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    P, AUX, feeds = mini
    results = []
    for graphs in ('0', '1'):
        monkeypatch.setenv('SNIPER_HIP_GRAPHS', graphs)
        sym = _mini_graph(mx, _G, _A)
        ex = Executor(sym, _SHAPES, True, _fixed(sym))
        assert ex.use_graphs == (graphs == '1')
        (gd,) = [s for s in ex.steps if type(s).__name__ == 'DeformableConvolutionStep']
        assert (gd.groups, gd.C // gd.groups, gd.dg) == (_G, 8, _DG) and gd.col is None
        ex.set_params(P, AUX)
        start = {k: p.master.clone() for k, p in ex.params.items()}
        outs = []
        for i, feed in enumerate(feeds):
            o = ex.forward_backward(feed)
            outs.append([t.clone() for t in o])
            ex.update(lr=1e-4 * (i + 1), wd=1e-3, momentum=0.9)
        torch.cuda.synchronize()
        if graphs == '1':
            assert ex._graph_fb is not None and ex._graph_up is not None, 'hipGraph capture did not happen'
        results.append((outs, {k: p.master.clone() for k, p in ex.params.items()}))
    (oe, pe), (og, pg) = results
    for a, b in zip(oe, og):
        for x, y in zip(a, b):
            assert torch.isfinite(x).all() and torch.equal(x, y), 'graph vs eager outputs'
    for k in pe:
        assert torch.equal(pe[k], pg[k]), 'graph vs eager ' + k
    for k in (_DW, 'stage4_unit1_offset_weight', 'stage4_unit1_offset_bias', 'stage3_unit1_conv2_weight'):
        assert not torch.equal(pe[k], start[k]), 'not updated: ' + k


def test_grouped_deformable_graph_gradients_vs_dense_twin(monkeypatch, mini):
    """One training step of the mini graph against oracle/graph_cpu.py, teacher-forced like test_gpu_engine._forced_parity.  The CPU
    graph contracts a deformable convolution densely, so it evaluates the DENSE TWIN: the same graph with num_group = 1 and the
    block-diagonal expansion of the grouped weights; the device's weight gradient is compared with the twin's diagonal blocks.
    tol_grad = 1e-2 (relative L2), 1.5 x that for the `_offset_` parameters as in _forced_parity."""
    import sniper_amd.mx as mx
    from oracle import graph_cpu
    from sniper_amd.engine.executor import Executor
    P, AUX, feeds = mini
    tol_fwd, tol_grad = 2e-3, 1e-2
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', '0')
    sym = _mini_graph(mx, _G, _A)
    ex = Executor(sym, _SHAPES, True, _fixed(sym))
    ex.set_params(P, AUX)
    inp = feeds[0]
    outs = ex.forward(inp, is_train=True)
    dev_vals = {}
    for st in ex.steps:
        y = getattr(st, 'y', None)
        kind = type(st).__name__
        if y is None or y.t is None or (kind == 'BatchNormStep' and getattr(st, 'act', 0)) or \
                getattr(st, 'fused_residual', None) is not None or getattr(st, 'fold_bn', None) is not None or \
                (kind == 'BatchNormStep' and getattr(st, 'folded_into', None) is not None and not getattr(st, 'act', 0)):
            continue            # (see _forced_parity: these hold the tensor of a later node)
        t = y.t.float()
        if y.fmt == 'act' and len(y.shape) == 4:
            t = t.permute(0, 3, 1, 2)
        if int(np.prod(y.shape)) != t.numel():
            continue
        dev_vals[st.node.name] = t.reshape(y.shape).cpu().numpy()
    assert 'stage4_unit1_conv2' in dev_vals and 'stage4_unit1_offset' in dev_vals
    assert float(np.abs(dev_vals['stage4_unit1_offset']).max()) > 0.25, 'the offsets of this test are too small to deform anything'
    ex.backward()
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    # the dense twin
    Cg = _MID // _G
    Pd = dict(P)
    dense = np.zeros((_MID, _MID, 3, 3), np.float32)
    for g in range(_G):
        dense[g * Cg:(g + 1) * Cg, g * Cg:(g + 1) * Cg] = P[_DW][g * Cg:(g + 1) * Cg]
    Pd[_DW] = dense
    twin = _mini_graph(mx, 1, _A)
    want, wgrads = graph_cpu.run(twin, Pd, AUX, inp, fork_ops=False, fp16_storage=True, force=dev_vals)
    le = graph_cpu.run.local_err
    assert len(le) > 0.8 * len(dev_vals) and 'stage4_unit1_conv2' in le
    worst = max(le, key=le.get)
    assert le[worst] <= tol_fwd, 'forward mismatch %.5f at node %s; all > tol: %s' % (
        le[worst], worst, [(k, round(v, 5)) for k, v in le.items() if v > tol_fwd])
    for g, w in zip(got, want):
        assert_close(g, w, 1e-2, 1e-2 * np.abs(w).max() + 1e-5, 'graph output')
    bad, checked = [], 0
    for name, p in ex.params.items():
        if not p.trainable:
            continue
        g, w = p.to_reference(p.grad.detach().cpu().numpy()), wgrads[name]
        if name == _DW:
            w = np.concatenate([w[i * Cg:(i + 1) * Cg, i * Cg:(i + 1) * Cg] for i in range(_G)], 0)      # the diagonal blocks
        assert g.shape == w.shape, name
        rel = float(np.linalg.norm(g.astype(np.float64) - w) / (np.linalg.norm(w) + 1e-20))
        print('%-36s relL2 %.5f' % (name, rel))
        if not rel <= (1.5 * tol_grad if '_offset_' in name and 'stage4' in name else tol_grad):
            bad.append((name, rel))
        checked += 1
    assert not bad, bad
    # 2 units x (3 convolutions + 3 BatchNorms x 2) + sc + sc_bn x 2 + offset weight and bias + 3 RPN layers x 2
    assert checked == 2 * 9 + 3 + 2 + 6, checked


def test_resnext101_dcn_trainer_steps():
    """Three optimizer steps of Trainer(cfg=resnext101_e2e_dcn(2)): finite losses; the three grouped deformable weights and the three
    offset layers (zero at the start) moved, the frozen stage 1 did not."""
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=2, n_images=8, cfg=cfgmod.resnext101_e2e_dcn(2))
    ex = tr.mod.exe
    steps = [s for s in ex.steps if type(s).__name__ == 'DeformableConvolutionStep']
    assert len(steps) == 3 and all(s.groups == 64 and s.dg == 4 and s.col is None for s in steps)
    moving = ['stage4_unit%d_%s' % (u, n) for u in (1, 2, 3) for n in ('conv2_weight', 'offset_weight', 'offset_bias')]
    names = moving + ['stage1_unit2_conv2_weight']
    before = {n: ex.params[n].master.clone() for n in names}
    for u in (1, 2, 3):
        assert not before['stage4_unit%d_offset_weight' % u].any() and not before['stage4_unit%d_offset_bias' % u].any()
    for _ in range(3):
        outs = tr.step()
        torch.cuda.synchronize()
        for o in outs:
            assert np.isfinite(o.asnumpy()).all()
        tr.next_batch()
    for n in names:
        assert torch.equal(before[n], ex.params[n].master) == n.startswith('stage1'), n
        assert torch.isfinite(ex.params[n].master).all(), n
