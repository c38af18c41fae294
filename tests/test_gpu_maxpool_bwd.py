"""-m gpu: the max-pool backward kernel (sn_maxpool_bwd, csrc/nn_ops.hip) against torch's CPU autograd bit for bit, its write-once /
accumulate / aliasing / determinism / argument contracts, and the path it opens: a small ResNet-style graph that trains its stem and a
stage-1-style pair of units (network.FIXED_PARAMS = []) teacher-forced against oracle/graph_cpu.py, under hipGraph replay, with
per-layer weight gradients, and two steps of Trainer(fixed_params=[])."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

pytestmark = pytest.mark.gpu

from gpu_util import assert_close, dev, f16r, from_nhwc, to_nhwc_f16  # noqa: E402

# (N, C, H, W, k, stride, pad)
_SHAPES = [
    (2, 64, 18, 14, 3, 2, 1),        # the forward test's shape
    (1, 8, 7, 9, 3, 2, 1),           # odd sides, one lane per pixel
    (2, 72, 5, 5, 3, 2, 1),          # C not a multiple of 64
    (1, 16, 8, 8, 2, 2, 0),          # disjoint windows
    (1, 8, 9, 9, 3, 1, 1),           # nine windows per element
    (1, 64, 37, 70, 3, 2, 1),        # sides that are not multiples of any tile
    (1, 64, 256, 256, 3, 2, 1),      # one chip's real geometry
    (1, 72, 70, 75, 3, 2, 1),        # the 3/2/1 kernel's tile is 32 x 32 pixels x 64 channels: three tiles each way (32, 32, 6 rows;
    #                                  32, 32, 11 columns) and a second channel chunk with one lane of eight in use
]
_CASES = {}


def _hip():
    from sniper_amd import hip
    return hip


def _case(shape):
    """inputs, torch's CPU gradient and the tied share of one shape -- computed once, shared by the tests, never written to"""
    if shape not in _CASES:
        N, C, H, W, k, s, p = shape
        rs = np.random.RandomState(sum(shape) + 31 * C)
        x = np.maximum(np.round(2 * rs.standard_normal((N, C, H, W))) / 2, 0).astype(np.float32)
        xt = torch.from_numpy(x).requires_grad_(True)
        y = Fnn.max_pool2d(xt, k, s, p)
        dy = (np.round(16 * rs.standard_normal(tuple(y.shape))) / 64).astype(np.float32)
        y.backward(torch.from_numpy(dy))
        want = xt.grad.numpy()
        assert np.array_equal(f16r(x), x) and np.array_equal(f16r(dy), dy) and np.array_equal(f16r(want), want)
        # windows whose maximum is held by two or more valid positions (padding, here -1 under a non-negative x, is no candidate)
        cols = Fnn.unfold(Fnn.pad(torch.from_numpy(x), (p, p, p, p), value=-1.0), k, 1, 0, s).reshape(N, C, k * k, -1)
        tied = float(((cols == cols.max(2, keepdim=True).values).sum(2) >= 2).float().mean())
        for a in (x, dy, want):
            a.setflags(write=False)
        _CASES[shape] = (x, dy, want, tied)
    return _CASES[shape]


def _run(shape, acc=None, dx=None, xd=None, dyd=None):
    hip = _hip()
    N, C, H, W, k, s, p = shape
    x, dy, _, _ = _case(shape)
    xd = to_nhwc_f16(x) if xd is None else xd
    dyd = to_nhwc_f16(dy) if dyd is None else dyd
    if dx is None:
        dx = torch.full((N, H, W, C), float('nan'), dtype=torch.float16, device=dev())
    hip.call('sn_maxpool_bwd', dyd, xd, acc, dx, N, H, W, C, k, s, p, hip.stream())
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize('shape', _SHAPES)
def test_maxpool_bwd_equals_torch_cpu_autograd(shape):
    """dx after rounding to fp16 == torch's CPU gradient of F.max_pool2d, exactly: x = relu(round(2 randn) / 2) ties the maximum of
    about three windows in ten (asserted >= 0.2, so the first-position rule is what is tested) and every fp32 sum of
    dy = round(16 randn) / 64 values is fp16-exact in any order.  dx starts as NaN: every element is written (write-once)."""
    x, dy, want, tied = _case(shape)
    print('%s: tied windows %.3f' % (shape, tied))
    assert tied >= 0.2, 'only %.3f of the windows have a tied maximum: the tie rule is not tested' % tied
    dx = _run(shape)
    assert not torch.isnan(dx).any(), 'dx keeps %d of its NaNs: not every element was written' % int(torch.isnan(dx).sum())
    assert_close(from_nhwc(dx), want, 0, 0, 'maxpool bwd %s' % (shape,))


@pytest.mark.parametrize('shape', [_SHAPES[0], _SHAPES[4], _SHAPES[7]])
def test_maxpool_bwd_accumulate_alias_and_determinism(shape):
    N, C, H, W, k, s, p = shape
    x, dy, want, _ = _case(shape)
    rs = np.random.RandomState(5)
    acc = rs.standard_normal((N, C, H, W)).astype(np.float16)
    accd = to_nhwc_f16(acc.astype(np.float32))
    want_acc = (want + acc.astype(np.float32)).astype(np.float16).astype(np.float32)      # fp32 sum (exact here), one rounding
    apart = _run(shape, acc=accd)
    assert_close(from_nhwc(apart), want_acc, 0, 0, 'maxpool bwd + accumulate')
    alias = accd.clone()
    _run(shape, acc=alias, dx=alias)
    assert torch.equal(alias, apart), 'accumulate aliased to dx differs from the separate tensor'
    assert torch.equal(_run(shape, acc=accd), apart) and torch.equal(_run(shape), _run(shape)), 'two calls differ'


def test_maxpool_bwd_argument_errors_leave_dx_untouched():
    from sniper_amd._lib import SniperHipError
    hip = _hip()
    N, H, W = 1, 8, 8
    x = torch.zeros((N, H, W, 16), dtype=torch.float16, device=dev())
    dy = torch.zeros((N, H, W, 16), dtype=torch.float16, device=dev())
    dx = torch.full((N, H, W, 16), 7.0, dtype=torch.float16, device=dev())

    def call(dy=dy, x=x, dx=dx, C=16, k=3, s=2, p=1):
        hip.call('sn_maxpool_bwd', dy, x, None, dx, N, H, W, C, k, s, p, hip.stream())

    for bad in (dict(dy=None), dict(x=None), dict(dx=None), dict(C=12), dict(k=3, s=4), dict(k=3, s=1, p=2), dict(k=8, s=2, p=1),
                dict(k=2, s=2, p=2), dict(s=0), dict(p=-1)):
        with pytest.raises(SniperHipError):
            call(**bad)
    torch.cuda.synchronize()
    assert float((dx.float() - 7.0).abs().max()) == 0.0, 'a refused call wrote dx'
    call()
    torch.cuda.synchronize()
    assert float(dx.float().abs().max()) == 0.0


# ---- the unfrozen small graph ----------------------------------------------------------------------------------------------------
def _full_trunk_graph(mx, A=3):
    """bn_data -> conv0 7x7/2 -> bn0 -> ReLU -> max pool 3/2/1 -> a stage-1-style projection unit 64 -> 256 -> an identity unit -> an
    RPN-style head (SoftmaxOutput + smooth-L1 MakeLoss).  Every BatchNorm is use_global_stats=True with trainable gamma / beta: the
    reference's stem and stage-1 form."""
    data = mx.sym.Variable('data')
    label, target, weight = mx.sym.Variable('label'), mx.sym.Variable('bbox_target'), mx.sym.Variable('bbox_weight')
    x = mx.sym.BatchNorm(data=data, name='bn_data', fix_gamma=True, eps=2e-5, use_global_stats=True)
    x = mx.sym.Convolution(data=x, name='conv0', num_filter=64, kernel=(7, 7), stride=(2, 2), pad=(3, 3), no_bias=True)
    x = mx.sym.Cast(data=x, dtype=np.float16)
    x = mx.sym.BatchNorm(data=x, name='bn0', fix_gamma=False, eps=2e-5, use_global_stats=True)
    x = mx.sym.Activation(data=x, act_type='relu', name='relu0')
    x = mx.sym.Pooling(data=x, kernel=(3, 3), stride=(2, 2), pad=(1, 1), pool_type='max', name='pool0')

    def bn_relu(x, name):
        y = mx.sym.BatchNorm(data=x, name=name, fix_gamma=False, eps=2e-5, use_global_stats=True)
        return mx.sym.Activation(data=y, act_type='relu', name=name + '_relu')

    def unit(x, nf, match, name):
        a1 = bn_relu(x, name + '_bn1')
        c1 = mx.sym.Convolution(data=a1, name=name + '_conv1', num_filter=nf // 4, kernel=(1, 1), no_bias=True)
        c2 = mx.sym.Convolution(data=bn_relu(c1, name + '_bn2'), name=name + '_conv2', num_filter=nf // 4, kernel=(3, 3), pad=(1, 1),
                                no_bias=True)
        c3 = mx.sym.Convolution(data=bn_relu(c2, name + '_bn3'), name=name + '_conv3', num_filter=nf, kernel=(1, 1), no_bias=True)
        sc = x if match else mx.sym.Convolution(data=a1, name=name + '_sc', num_filter=nf, kernel=(1, 1), no_bias=True)
        return c3 + sc

    u1 = unit(x, 256, False, 'stage1_unit1')
    u2 = unit(u1, 256, True, 'stage1_unit2')
    top = mx.sym.Cast(data=bn_relu(u2, 'bn1'), dtype=np.float32)
    r = mx.sym.Activation(data=mx.sym.Convolution(data=top, kernel=(3, 3), pad=(1, 1), num_filter=64, name='rpn_conv_3x3'),
                          act_type='relu', name='rpn_relu')
    cls = mx.sym.Convolution(data=r, kernel=(1, 1), num_filter=2 * A, name='rpn_cls_score')
    box = mx.sym.Convolution(data=r, kernel=(1, 1), num_filter=4 * A, name='rpn_bbox_pred')
    cls_r = mx.sym.Reshape(data=cls, shape=(0, 2, -1, 0), name='rpn_cls_score_reshape')
    prob = mx.sym.SoftmaxOutput(data=cls_r, label=label, multi_output=True, normalization='valid', use_ignore=True,
                                ignore_label=-1, name='rpn_cls_prob', grad_scale=100.0)
    l1 = weight * mx.sym.smooth_l1(name='rpn_bbox_loss_', scalar=1.0, data=(box - target))
    loss = mx.sym.MakeLoss(name='rpn_bbox_loss', data=l1, grad_scale=3 * 100.0 / 64.0)
    return mx.sym.Group([prob, loss])


def _shapes(B, H, W, A=3):
    fh, fw = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1        # conv0 7x7/2 pad 3, then pooling 3/2/1
    return dict(data=(B, 3, H, W), label=(B, A * fh * fw), bbox_target=(B, 4 * A, fh, fw), bbox_weight=(B, 4 * A, fh, fw))


def _feed(rs, shapes, scale=2.0):
    return dict(data=f16r(rs.standard_normal(shapes['data']) * scale),
                label=rs.choice([-1, 0, 1], size=shapes['label'], p=[0.5, 0.3, 0.2]).astype(np.float32),
                bbox_target=rs.standard_normal(shapes['bbox_target']).astype(np.float32),
                bbox_weight=(rs.uniform(size=shapes['bbox_weight']) < 0.2).astype(np.float32))


def _params(sym, shapes, rs):
    from test_gpu_engine import _init_params
    P, AUX = _init_params(sym, shapes, rs, bn_gamma=(0.5, 1.0), bn_beta=(-0.2, 0.4))
    P['bn_data_gamma'][:] = 1.0
    P['bn_data_beta'][:] = 0.0
    AUX['bn_data_moving_mean'][:] = 0.0
    AUX['bn_data_moving_var'][:] = 1.0 - 2e-5          # bn_data == identity: the image stays fp16-representable
    return P, AUX


def _executor(monkeypatch, sym, shapes, graphs='0', defer=None):
    from sniper_amd.engine.executor import Executor
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', graphs)
    if defer is None:
        monkeypatch.delenv('SNIPER_WGRAD_DEFER', raising=False)
    else:
        monkeypatch.setenv('SNIPER_WGRAD_DEFER', defer)
    ex = Executor(sym, shapes, True, [])                # fixed_param_names = []
    pool = [s for s in ex.steps if type(s).__name__ == 'PoolingStep'][0]
    assert pool.kind == 'max' and pool.x.needs_grad
    return ex


def _forced(sym, ex, P, AUX, inp, tol_fwd, tol_grad):
    """test_gpu_engine._forced_parity without its proposal steps: one training step against oracle/graph_cpu.py, every operator of
    the CPU evaluation fed the device's input activations, gradients through the CPU operators.  -> {parameter: relative L2}."""
    from oracle import graph_cpu
    ex.set_params(P, AUX)
    outs = ex.forward(inp, is_train=True)
    dev_vals = {}
    for st in ex.steps:
        y = getattr(st, 'y', None)
        kind = type(st).__name__
        if y is None or y.t is None or (kind == 'BatchNormStep' and getattr(st, 'act', 0)) or \
                getattr(st, 'fused_residual', None) is not None or getattr(st, 'fold_bn', None) is not None:
            continue            # (a BatchNorm fused with its ReLU is forced at the activation node, a convolution that absorbed
            #                     the residual add at the add node)
        t = y.t.float()
        if y.fmt == 'act' and len(y.shape) == 4:
            t = t.permute(0, 3, 1, 2)
        if int(np.prod(y.shape)) != t.numel():
            continue
        dev_vals[st.node.name] = t.reshape(y.shape).cpu().numpy()
    assert 'pool0' in dev_vals and 'relu0' in dev_vals
    ex.backward()
    torch.cuda.synchronize()
    got = [o.cpu().numpy() for o in outs]
    assert all(np.isfinite(g).all() for g in got)
    want, wgrads = graph_cpu.run(sym, P, AUX, inp, fork_ops=False, fp16_storage=True, force=dev_vals)
    le = graph_cpu.run.local_err
    assert len(le) > 0.8 * len(dev_vals)
    worst = max(le, key=le.get)
    print('forward: worst node %s relL2 %.6f' % (worst, le[worst]))
    assert le[worst] <= tol_fwd, 'forward mismatch %.5f at node %s (tolerance %.1e); all > tol: %s' % (
        le[worst], worst, tol_fwd, [(k, round(v, 5)) for k, v in le.items() if v > tol_fwd])
    for g, w in zip(got, want):
        assert_close(g, w, 1e-2, 1e-2 * np.abs(w).max() + 1e-5, 'graph output')
    rels = {}
    for name, p in ex.params.items():
        if not p.trainable:
            continue
        g, w = p.to_reference(p.grad.detach().cpu().numpy()), wgrads[name]
        rels[name] = float(np.linalg.norm(g.astype(np.float64) - w) / (np.linalg.norm(w) + 1e-20))
        print('%-36s relL2 %.5f' % (name, rels[name]))
    bad = {k: v for k, v in rels.items() if not v <= tol_grad}
    assert not bad, '%d of %d parameter gradients beyond %.1e: %s' % (len(bad), len(rels), tol_grad, bad)
    return rels


@pytest.mark.parametrize('H,W', [(64, 64), (70, 60)])
def test_unfrozen_small_graph_parity_vs_cpu_reference_ops(monkeypatch, H, W):
    """fixed_param_names = []: conv0, bn0 and both units train through the max-pool backward.  Per-node forward <= 2e-3 and every
    parameter gradient <= 1e-2 (relative L2) against the teacher-forced CPU graph -- conv0_weight, bn0_gamma, bn0_beta among them;
    bn_data stays frozen, and an SGD step moves every other parameter.  (70, 60): the pool's input is 35 x 30."""
    import sniper_amd.mx as mx
    sym = _full_trunk_graph(mx)
    shapes = _shapes(2, H, W)
    ex = _executor(monkeypatch, sym, shapes)
    rs = np.random.RandomState(H + W)
    P, AUX = _params(sym, shapes, rs)
    rels = _forced(sym, ex, P, AUX, _feed(rs, shapes), tol_fwd=2e-3, tol_grad=1e-2)
    names = [n for n in sym.list_arguments() if n not in shapes]
    assert not ex.params['bn_data_gamma'].trainable and not ex.params['bn_data_beta'].trainable
    assert sorted(rels) == sorted(n for n in names if not n.startswith('bn_data_'))
    assert {'conv0_weight', 'bn0_gamma', 'bn0_beta', 'stage1_unit1_sc_weight', 'stage1_unit2_bn1_beta'} <= set(rels)
    before = {n: ex.params[n].master.clone() for n in names}
    ex.update(lr=1e-3, wd=0.0, momentum=0.9)
    torch.cuda.synchronize()
    for n in names:
        assert torch.isfinite(ex.params[n].master).all(), n
        assert torch.equal(before[n], ex.params[n].master) == n.startswith('bn_data_'), n


def _five_steps(monkeypatch, graphs, defer, cache={}):
    import sniper_amd.mx as mx
    sym = _full_trunk_graph(mx)
    shapes = _shapes(2, 64, 64)
    ex = _executor(monkeypatch, sym, shapes, graphs, defer)
    assert ex.use_graphs == (graphs == '1') and ex.defer_wgrads == (defer != '0')
    if not cache:
        rs = np.random.RandomState(11)
        cache['P'], cache['AUX'] = _params(sym, shapes, rs)
        cache['feeds'] = [_feed(rs, shapes) for _ in range(5)]
    ex.set_params(cache['P'], cache['AUX'])
    start = {k: p.master.clone() for k, p in ex.params.items()}
    outs = []
    for i, feed in enumerate(cache['feeds']):
        o = ex.forward_backward(feed)
        outs.append([t.clone() for t in o])
        ex.update(lr=1e-4 * (i + 1), wd=1e-3, momentum=0.9)
    torch.cuda.synchronize()
    if graphs == '1':
        assert ex._graph_fb is not None and ex._graph_up is not None, 'hipGraph capture did not happen'
    return (outs, {k: p.grad.clone() for k, p in ex.params.items() if p.trainable}, {k: p.master.clone() for k, p in ex.params.items()},
            start)


def _same_bits(a, b, what):
    (oa, ga, pa, start), (ob, gb, pb, _) = a, b
    for x, y in zip(oa, ob):
        for s, t in zip(x, y):
            assert torch.isfinite(s).all() and torch.equal(s, t), what + ': outputs'
    for k in ga:
        assert torch.equal(ga[k], gb[k]), '%s: gradient of %s' % (what, k)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), '%s: %s' % (what, k)
    for k in ('conv0_weight', 'bn0_gamma', 'bn0_beta', 'stage1_unit1_conv2_weight'):
        assert not torch.equal(pa[k], start[k]), 'not updated: ' + k


def test_unfrozen_graph_replay_is_bit_equal_to_eager(monkeypatch):
    """five steps eagerly and five with the captured forward+backward / optimizer graphs (the weight-gradient work of the stem and
    the stage-1 layers now in them): outputs, the last gradients and the updated parameters are the same bits."""
    _same_bits(_five_steps(monkeypatch, '0', None), _five_steps(monkeypatch, '1', None), 'graph vs eager')


def test_unfrozen_graph_per_layer_weight_gradients_are_bit_equal_to_deferred(monkeypatch):
    """SNIPER_WGRAD_DEFER=0 (a launch per layer at the layer's backward) against the default (batched tables), eagerly"""
    _same_bits(_five_steps(monkeypatch, '0', None), _five_steps(monkeypatch, '0', '0'), 'per layer vs deferred')


def test_trainer_with_empty_fixed_params_trains_the_whole_trunk():
    """Trainer(batch_images=2, fixed_params=[]): two steps at a learning rate a random initialisation survives.  Finite outputs;
    conv0, bn0 and stage 1 moved; bn_data and bn0's moving statistics did not."""
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=2, n_images=8, fixed_params=[])
    tr.mod.init_optimizer(optimizer='sgd', optimizer_params={'learning_rate': 2e-5, 'momentum': 0.9, 'wd': 1e-4})
    ex = tr.mod.exe
    moved = ['conv0_weight', 'bn0_gamma', 'stage1_unit1_conv1_weight']
    still = ['bn_data_gamma', 'bn_data_beta']
    aux = ['bn0_moving_mean', 'bn0_moving_var', 'bn_data_moving_mean', 'bn_data_moving_var']
    assert all(ex.params[n].trainable for n in moved) and not any(ex.params[n].trainable for n in still)
    before = {n: ex.params[n].master.clone() for n in moved + still}
    before_aux = {n: ex.aux[n].clone() for n in aux}
    for _ in range(2):
        outs = tr.step()
        torch.cuda.synchronize()
        for o in outs:
            assert np.isfinite(o.asnumpy()).all()
        tr.next_batch()
    for n in moved:
        assert torch.isfinite(ex.params[n].master).all() and not torch.equal(before[n], ex.params[n].master), n
    for n in still:
        assert torch.equal(before[n], ex.params[n].master), n
    for n in aux:
        assert torch.equal(before_aux[n], ex.aux[n]), n
