"""-m gpu: grouped convolution (csrc/gconv.hip) -- the kernels against torch on the CPU, the weight gradient's bit-reproducibility,
the lowered ResNeXt-101 training step against the CPU graph oracle, hipGraph replay of a small grouped graph, the test-time
BatchNorm fold into a grouped layer, and two optimizer steps of the resnext101_e2e preset."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

pytestmark = pytest.mark.gpu

from gpu_util import assert_close, dev, f16r, from_nhwc, to_nhwc_f16, w_to_otI  # noqa: E402

# (N, C, O, groups, H, W, K, stride, pad, dil, extra output pitch)
_FAST = [
    (2, 64, 64, 16, 12, 10, 3, 1, 1, 1, 0),        # Cg = 4
    (2, 64, 64, 16, 11, 13, 3, 2, 1, 1, 0),        # Cg = 4, stride 2, odd extents
    (2, 64, 64, 8, 11, 13, 3, 1, 1, 1, 0),         # Cg = 8
    (1, 128, 128, 16, 12, 9, 3, 2, 1, 1, 0),       # Cg = 8, stride 2
    (2, 96, 96, 6, 11, 13, 3, 1, 1, 1, 0),         # Cg = 16: three slabs (waves per workgroup = 1)
    (2, 64, 64, 4, 10, 12, 3, 2, 1, 1, 0),         # Cg = 16, stride 2
    (2, 64, 64, 2, 11, 13, 3, 1, 1, 1, 0),         # Cg = 32
    (1, 128, 128, 4, 9, 14, 3, 2, 1, 1, 0),        # Cg = 32, stride 2
    (2, 64, 64, 2, 11, 13, 3, 1, 2, 2, 0),         # Cg = 32, dilation 2 (stage 4)
    (2, 64, 64, 8, 11, 13, 3, 1, 1, 1, 24),        # output pitch larger than O
    (2, 256, 256, 64, 7, 9, 3, 1, 1, 1, 0),        # the stage-1 ResNeXt layer: 64 groups of 4
    (2, 64, 64, 8, 11, 13, 1, 1, 0, 1, 0),         # 1x1 grouped layer
    (2, 64, 64, 2, 9, 8, 1, 2, 0, 1, 0),           # 1x1, Cg = 32, stride 2
]
_PLAIN = [
    (2, 24, 48, 4, 11, 13, 3, 1, 1, 1, 0),         # Cg = 6, Og = 12
    (2, 24, 24, 8, 11, 13, 5, 1, 2, 1, 0),         # Cg = Og = 3 at 5x5
    (1, 16, 32, 2, 9, 7, 3, 2, 1, 1, 8),           # Cg = 8 != Og = 16, stride 2, padded pitch
]


def _hip():
    from sniper_amd import hip
    return hip


@pytest.mark.parametrize('N,C,O,g,H,W,K,s,p,d,extra', _FAST + _PLAIN)
def test_grouped_conv_vs_torch(N, C, O, g, H, W, K, s, p, d, extra):
    """forward (plain, then bias + ReLU), data gradient (plain, then `accumulate` aliasing dx: 2x), weight gradient (three runs
    into zeroed buffers: the same bits), against torch.nn.functional.conv2d(groups=g) on fp16-rounded operands."""
    hip = _hip()
    Cg = C // g
    rs = np.random.RandomState(C + 7 * g + s + K)
    x = rs.standard_normal((N, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((O, Cg, K, K)) / np.sqrt(Cg * K * K)).astype(np.float32)
    b = rs.standard_normal((O,)).astype(np.float32)
    xt, wt = torch.from_numpy(f16r(x)).requires_grad_(True), torch.from_numpy(f16r(w)).requires_grad_(True)
    y = Fnn.conv2d(xt, wt, None, s, p, d, groups=g)
    dy = rs.standard_normal(tuple(y.shape)).astype(np.float32)
    y.backward(torch.from_numpy(f16r(dy)))
    want_y = y.detach().numpy()
    Ho, Wo = y.shape[2], y.shape[3]
    xd = to_nhwc_f16(x)
    wd = torch.from_numpy(w_to_otI(w)).to(dev()).half().contiguous()
    bd = torch.from_numpy(b).to(dev())
    ops = O + extra
    yd = torch.full((N, Ho, Wo, ops), 7.0, dtype=torch.float16, device=dev())
    hip.call('sn_gconv_fwd', xd, wd, None, yd, N, H, W, C, C, O, ops, g, K, K, s, p, d, 0, 0, hip.stream())
    assert_close(from_nhwc(yd[..., :O]), want_y, 1e-2, 1e-2 * np.abs(want_y).max(), 'gconv fwd')
    if extra:
        assert float((yd[..., O:].float() - 7.0).abs().max()) == 0.0, 'the padding of the output pitch was written'
    hip.call('sn_gconv_fwd', xd, wd, bd, yd, N, H, W, C, C, O, ops, g, K, K, s, p, d, 1, 0, hip.stream())
    want_r = np.maximum(want_y + b.reshape(1, O, 1, 1), 0)
    assert_close(from_nhwc(yd[..., :O]), want_r, 1e-2, 1e-2 * np.abs(want_r).max(), 'gconv fwd bias relu')
    # data gradient; dy with the same padded pitch
    dyd = torch.zeros((N, Ho, Wo, ops), dtype=torch.float16, device=dev())
    dyd[..., :O] = to_nhwc_f16(dy)
    dx = torch.full((N, H, W, C), 7.0, dtype=torch.float16, device=dev())
    hip.call('sn_gconv_dgrad', dyd, wd, None, dx, N, H, W, C, O, ops, C, C, g, K, K, s, p, d, hip.stream())
    want_dx = xt.grad.numpy()
    assert_close(from_nhwc(dx), want_dx, 1e-2, 1e-2 * np.abs(want_dx).max(), 'gconv dgrad')
    hip.call('sn_gconv_dgrad', dyd, wd, dx, dx, N, H, W, C, O, ops, C, C, g, K, K, s, p, d, hip.stream())
    assert_close(from_nhwc(dx), 2 * want_dx, 1e-2, 1e-2 * np.abs(2 * want_dx).max(), 'gconv dgrad accumulate')
    # weight gradient
    need = hip.query('sn_gconv_wgrad_workspace_bytes', N, H, W, C, O, g, K, K, s, p, d)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    runs = []
    for rep in range(3):
        dw = torch.zeros((O, K * K, Cg), dtype=torch.float32, device=dev())
        hip.call('sn_gconv_wgrad', dyd, xd, dw, N, H, W, C, O, ops, C, g, K, K, s, p, d, ws, need, hip.stream())
        runs.append(dw.clone())
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    want_dw = w_to_otI(wt.grad.numpy())
    assert_close(dw.cpu().numpy(), want_dw, 1e-2, 1e-2 * np.abs(want_dw).max(), 'gconv wgrad')
    hip.call('sn_gconv_wgrad', dyd, xd, dw, N, H, W, C, O, ops, C, g, K, K, s, p, d, ws, need, hip.stream())     # += into dw
    assert_close(dw.cpu().numpy(), 2 * want_dw, 1e-2, 1e-2 * np.abs(2 * want_dw).max(), 'gconv wgrad accumulates')


# (C, O, groups) and the (N, H, W) of 3x3 / stride 1 / pad 1 problems whose pixel-block counts are 4, 8 and 11
_FINISH = [
    ('mfma', 64, 64, 2, [(1, 10, 10), (1, 15, 15), (2, 13, 13)]),        # Cg = 32: one block per 32-pixel chunk
    ('plain', 24, 48, 4, [(1, 15, 15), (2, 15, 16), (2, 18, 19)]),       # Cg = 6, Og = 12: blocks of about 64 pixels
]


def test_grouped_wgrad_partial_sum_block_counts():
    """The ordered finish of sn_gconv_wgrad (sn_partial_sum, shared with the depthwise weight gradient and the bias gradient) over
    every loop shape of its block walk, behind the MFMA and the plain kernel: pixel-block counts (the workspace query over 4 bytes
    x the weight count) below 8, a multiple of 8 and above 8 but no multiple; `dw +=` on a non-zero dw against the float64
    gradient, the same bits on a second call."""
    hip = _hip()
    for path, C, O, g, shapes in _FINISH:
        Cg, nw = C // g, O * 9 * (C // g)
        rs = np.random.RandomState(C + g)
        w = torch.zeros((O, Cg, 3, 3), dtype=torch.float64, requires_grad=True)
        dw0 = torch.from_numpy(rs.standard_normal((O, 9, Cg)).astype(np.float32)).to(dev())
        counts = []
        for (N, H, W) in shapes:
            x = rs.standard_normal((N, C, H, W)).astype(np.float32)
            dy = rs.standard_normal((N, O, H, W)).astype(np.float32)
            w.grad = None
            Fnn.conv2d(torch.from_numpy(f16r(x)).double(), w, None, 1, 1, 1, groups=g).backward(torch.from_numpy(f16r(dy)).double())
            want = dw0.double().cpu().numpy() + w.grad.numpy().transpose(0, 2, 3, 1).reshape(O, 9, Cg)
            xd, dyd = to_nhwc_f16(x), to_nhwc_f16(dy)
            need = hip.query('sn_gconv_wgrad_workspace_bytes', N, H, W, C, O, g, 3, 3, 1, 1, 1)
            counts.append(need // (4 * nw))
            ws = torch.empty(need, dtype=torch.uint8, device=dev())
            runs = []
            for rep in range(2):
                dw = dw0.clone()
                hip.call('sn_gconv_wgrad', dyd, xd, dw, N, H, W, C, O, O, C, g, 3, 3, 1, 1, 1, ws, need, hip.stream())
                runs.append(dw)
            assert torch.equal(runs[0], runs[1]), (path, N, H, W)
            assert_close(runs[0].cpu().numpy(), want, 1e-2, 1e-2 * np.abs(want).max(), 'gconv wgrad finish %s %dx%dx%d' % (path, N, H, W))
        assert counts == [4, 8, 11], (path, counts)
        assert any(b < 8 for b in counts) and any(b % 8 == 0 for b in counts) and any(b > 8 and b % 8 for b in counts), (path, counts)


def test_grouped_conv_fp32_output():
    """a head-style grouped layer whose consumer wants fp32: the plain kernel writes it"""
    hip = _hip()
    N, C, O, g, H, W = 2, 64, 64, 8, 6, 7
    rs = np.random.RandomState(3)
    x, w = rs.standard_normal((N, C, H, W)).astype(np.float32), (rs.standard_normal((O, C // g, 3, 3)) / 8).astype(np.float32)
    b = rs.standard_normal((O,)).astype(np.float32)
    want = Fnn.conv2d(torch.from_numpy(f16r(x)), torch.from_numpy(f16r(w)), torch.from_numpy(b), 1, 1, 1, groups=g).numpy()
    yd = torch.empty((N, H, W, O), dtype=torch.float32, device=dev())
    hip.call('sn_gconv_fwd', to_nhwc_f16(x), torch.from_numpy(w_to_otI(w)).to(dev()).half().contiguous(), torch.from_numpy(b).to(dev()),
             yd, N, H, W, C, C, O, O, g, 3, 3, 1, 1, 1, 0, 1, hip.stream())
    assert_close(from_nhwc(yd), want, 1e-3, 1e-3 * np.abs(want).max(), 'gconv fwd fp32')


def _resnext_executor(B):
    import os
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.symbols.faster import resnext_mx_101_e2e as rx
    from sniper_amd.train import fixed_param_names
    A, F = 21, 32
    cfg = cfgmod.resnext101_e2e(batch_images=B)
    sym = rx.resnext_mx_101_e2e(momentum=0.995).get_symbol_rcnn(cfg)
    shapes = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, A * F * F),
                  bbox_target=(B, 4 * A, F, F), bbox_weight=(B, 4 * A, F, F), gt_boxes=(B, 100, 5))
    os.environ['SNIPER_HIP_GRAPHS'] = '0'
    try:
        ex = Executor(sym, shapes, True, fixed_param_names(cfg, sym))
    finally:
        os.environ.pop('SNIPER_HIP_GRAPHS', None)
    return sym, ex, shapes, A, F


def test_resnext101_network_parity_vs_cpu_reference_ops():
    """The ResNeXt-101 64x4d training graph at 2 chips, teacher-forced against oracle/graph_cpu.py like the R101 test, with its
    tolerances: the 33 grouped 3x3 layers (Cg 4 / 8 / 16 / 32, the stride-2 openers of stages 2 and 3, the dilation-2 layers of
    stage 4) forward, data gradient and weight gradient, between stand-alone-statistics BatchNorms."""
    from test_gpu_engine import _forced_parity, _init_params, _train_inputs
    B = 2
    sym, ex, shapes, A, F = _resnext_executor(B)
    grouped = [s for s in ex.steps if type(s).__name__ == 'ConvolutionStep' and s.grouped]
    assert len(grouped) == 33
    rs = np.random.RandomState(13)
    P, AUX = _init_params(sym, shapes, rs, bn_gamma=(0.5, 1.0), bn_beta=(-0.2, 0.4))
    P['bn_data_gamma'][:] = 1.0
    AUX['bn_data_moving_mean'][:] = 0.0
    AUX['bn_data_moving_var'][:] = 1.0 - 2e-5      # bn_data == identity: the image stays fp16-representable
    P['bn_data_beta'][:] = 0.0
    inp = _train_inputs(rs, B, A, F)
    checked, _ = _forced_parity(sym, ex, P, AUX, inp, tol_fwd=2e-3, tol_grad=1e-2)
    # trainable: stages 2 - 4 (30 units x (3 convolutions + 3 BatchNorms x 2) + 3 openers x (sc + sc_bn x 2)) + the heads (rpn x 3,
    # conv_new_1, fc_new_1/2, cls_score, bbox_pred, offset: 9 layers with weight and bias)
    assert checked == 30 * 9 + 3 * 3 + 9 * 2, checked


def _grouped_mini_graph(mx, A=3):
    """frozen stem -> two ResNeXt units (grouped 3x3 with Cg = 8 on the matrix cores, stride 2 with projection shortcut; then
    Cg = 6 -> Og = 12 on the plain kernels) -> RPN head -> SoftmaxOutput + smooth-L1 MakeLoss"""
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

    def unit(x, mid, mid2, nf, groups, stride, match, name):
        c1 = mx.sym.Convolution(data=x, name=name + '_conv1', num_filter=mid, kernel=(1, 1), no_bias=True)
        c2 = mx.sym.Convolution(data=bn(c1, name + '_bn1'), name=name + '_conv2', num_filter=mid2, num_group=groups, kernel=(3, 3),
                                stride=(stride, stride), pad=(1, 1), no_bias=True)
        c3 = mx.sym.Convolution(data=bn(c2, name + '_bn2'), name=name + '_conv3', num_filter=nf, kernel=(1, 1), no_bias=True)
        sc = x if match else bn(mx.sym.Convolution(data=x, name=name + '_sc', num_filter=nf, kernel=(1, 1), stride=(stride, stride),
                                                   no_bias=True), name + '_sc_bn', relu=False)
        return mx.sym.Activation(data=bn(c3, name + '_bn3', relu=False) + sc, act_type='relu', name=name + '_relu')

    u1 = unit(x, 64, 64, 128, 8, 2, False, 'stage2_unit1')
    u2 = unit(u1, 48, 96, 128, 8, 1, True, 'stage2_unit2')
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


def test_grouped_graph_replay_is_bit_equal_to_eager(monkeypatch):
    """A small graph with grouped layers (fast path and plain path), five steps eagerly and five with the captured forward+backward
    / optimizer graphs: every launch of gconv.hip is deterministic and takes its scratch from the executor, so the outputs and the
    updated parameters are the same bits."""
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    A, B, S = 3, 2, 64
    F = S // 8
    shapes = dict(data=(B, 3, S, S), label=(B, A * F * F), bbox_target=(B, 4 * A, F, F), bbox_weight=(B, 4 * A, F, F))
    rs = np.random.RandomState(6)
    results = []
    for graphs in ('0', '1'):
        monkeypatch.setenv('SNIPER_HIP_GRAPHS', graphs)
        sym = _grouped_mini_graph(mx, A)
        fixed = [n for n in sym.list_arguments() if any(p in n for p in ('conv0', 'bn0', 'bn_data'))]
        ex = Executor(sym, shapes, True, fixed)
        assert ex.use_graphs == (graphs == '1')
        grouped = [s for s in ex.steps if type(s).__name__ == 'ConvolutionStep' and s.grouped]
        assert [(s.groups, s.C // s.groups, s.O // s.groups) for s in grouped] == [(8, 8, 8), (8, 6, 12)]
        if not results:
            args, _, auxs = sym.infer_shape(**shapes)
            P, AUX = {}, {}
            for name, shp in zip(sym.list_arguments(), args):
                if name not in shapes:
                    P[name] = rs.uniform(0.5, 1.5, shp).astype(np.float32) if name.endswith('_gamma') else \
                        (rs.standard_normal(shp) * (0.1 if len(shp) == 1 else np.sqrt(2.0 / np.prod(shp[1:])))).astype(np.float32)
            for name, shp in zip(sym.list_auxiliary_states(), auxs):
                AUX[name] = rs.uniform(0.5, 1.5, shp).astype(np.float32)
            feeds = [dict(data=(rs.standard_normal((B, 3, S, S)) * 2).astype(np.float32),
                          label=rs.choice([-1, 0, 1], size=(B, A * F * F), p=[0.5, 0.3, 0.2]).astype(np.float32),
                          bbox_target=rs.standard_normal((B, 4 * A, F, F)).astype(np.float32),
                          bbox_weight=(rs.uniform(size=(B, 4 * A, F, F)) < 0.2).astype(np.float32)) for _ in range(5)]
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
    for k in ('stage2_unit1_conv2_weight', 'stage2_unit2_conv2_weight'):
        assert not torch.equal(pe[k], start[k]), 'the grouped weights were not updated: ' + k


def test_batchnorm_folds_into_a_grouped_layer_at_test_time(monkeypatch):
    """test-time graph: grouped 3x3 -> BatchNorm -> ReLU -> 1x1 head.  The BatchNorm (+ ReLU) rides in the grouped layer's compact
    weights, bias and epilogue (ConvolutionStep.refold + sn_gconv_fwd's bias / ReLU); same result as the separate pass and as torch."""
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    N, C, g, H, W = 2, 64, 8, 9, 11
    data = mx.sym.Variable('data')
    y = mx.sym.Convolution(data=data, name='gc', num_filter=C, num_group=g, kernel=(3, 3), pad=(1, 1), no_bias=True)
    y = mx.sym.Activation(data=mx.sym.BatchNorm(data=y, name='gbn', fix_gamma=False, eps=2e-5, use_global_stats=True),
                          act_type='relu', name='grelu')
    sym = mx.sym.Group([mx.sym.Convolution(data=y, name='head', num_filter=8, kernel=(1, 1), no_bias=True)])
    rs = np.random.RandomState(8)
    x = f16r(rs.standard_normal((N, C, H, W)))
    P = dict(gc_weight=f16r(rs.standard_normal((C, C // g, 3, 3)) / 8), head_weight=f16r(rs.standard_normal((8, C, 1, 1)) / 8),
             gbn_gamma=rs.uniform(0.5, 1.5, C).astype(np.float32), gbn_beta=rs.standard_normal(C).astype(np.float32))
    AUX = dict(gbn_moving_mean=rs.standard_normal(C).astype(np.float32) * 0.1, gbn_moving_var=rs.uniform(0.5, 1.5, C).astype(np.float32))
    t = Fnn.conv2d(torch.from_numpy(x), torch.from_numpy(P['gc_weight']), None, 1, 1, 1, groups=g)
    t = Fnn.batch_norm(t, torch.from_numpy(AUX['gbn_moving_mean']), torch.from_numpy(AUX['gbn_moving_var']),
                       torch.from_numpy(P['gbn_gamma']), torch.from_numpy(P['gbn_beta']), False, 0.0, 2e-5)
    want = Fnn.conv2d(torch.relu(t), torch.from_numpy(P['head_weight'])).numpy()
    outs = []
    for fold in ('1', '0'):
        monkeypatch.setenv('SNIPER_INFER_FOLD_BN', fold)
        ex = Executor(sym, dict(data=(N, C, H, W)), False)
        gc = [s for s in ex.steps if s.node.name == 'gc'][0]
        assert gc.grouped and (gc.fold_bn is not None) == (fold == '1')
        ex.set_params(P, AUX)
        out = ex.forward(dict(data=x), is_train=False)[0]
        torch.cuda.synchronize()
        outs.append(out.float().cpu().numpy().reshape(want.shape))
        assert_close(outs[-1], want, 1e-2, 1e-2 * np.abs(want).max(), 'grouped layer with folded BatchNorm = %s' % fold)
    assert_close(outs[0], outs[1], 1e-2, 1e-2 * np.abs(want).max(), 'folded vs separate BatchNorm')


def test_resnext101_trainer_steps():
    """Two optimizer steps of Trainer(cfg=resnext101_e2e(2)): finite losses, and the trainable weights -- the grouped ones among them
    -- moved while the frozen stage 1 did not."""
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=2, n_images=8, cfg=cfgmod.resnext101_e2e(2))
    ex = tr.mod.exe
    names = ['stage1_unit2_conv2_weight', 'stage2_unit1_conv2_weight', 'stage3_unit7_conv2_weight', 'stage4_unit3_conv2_weight',
             'stage2_unit1_sc_bn_gamma', 'rpn_conv_3x3_weight']
    before = {n: ex.params[n].master.clone() for n in names}
    for _ in range(2):
        outs = tr.step()
        torch.cuda.synchronize()
        for o in outs:
            assert np.isfinite(o.asnumpy()).all()
        tr.next_batch()
    for n in names:
        same = torch.equal(before[n], ex.params[n].master)
        assert same == n.startswith('stage1'), n
        assert torch.isfinite(ex.params[n].master).all(), n
