"""-m gpu: dynamic loss scaling -- the loss-gradient kernels that read the scale from the device against the plain kernels called
with grad_scale * S (bit for bit), sn_grad_guard_scaled against its numpy restatement (tests/loss_scale_ref.py) over a trajectory of
back-offs and growths, the exactness of unscaling inside the guarded update, sn_aux_shadow, and then whole steps of a small graph,
eager and captured: a fixed dynamic scale against the static one, a forward overflow that leaves NOTHING changed (BatchNorm moving
statistics included), growth, a start far too high that finds its level, and the R101 Trainer."""
import numpy as np
import pytest
import torch

import loss_scale_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-7          # the active-path bound of the guarded update (tests/test_gpu_grad_guard.py)
SCALES = [2.0 ** -3, 1.0, 2.0 ** 7, 2.0 ** 15]


def _hip():
    from sniper_amd import hip
    return hip


def _ls(scale):
    t = torch.zeros(8, dtype=torch.float64, device=dev())
    t[0] = scale
    return t


def _padded(n, fill=-7.5, pad=8):
    """-> (buffer, 16-byte aligned view of n floats with `pad` floats of `fill` on both sides)"""
    buf = torch.full((n + 2 * pad,), fill, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0 and pad % 4 == 0
    return buf, buf[pad:pad + n]


# ------------------------------------------------------------------------------------------------
# 1. the scaled loss kernels
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def softmax_cases():
    """probabilities and labels of the two paths, made once: rows (inner == 1: two row blocks, the second of 3 rows = 243 floats with
    a 3-float tail) and strided; labels with ignored entries, and all of them ignored"""
    rs = np.random.RandomState(11)
    out = {}
    for name, (outer, K, inner) in (('rows', (67, 81, 1)), ('strided', (2, 2, 37))):
        x = rs.standard_normal((outer, K, inner)).astype(np.float32) * 3
        e = np.exp(x - x.max(axis=1, keepdims=True))
        p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        label = rs.randint(0, K, (outer, inner)).astype(np.float32)
        label[rs.uniform(size=label.shape) < 0.3] = -1.0
        assert (label == -1).any() and (label != -1).any()
        out[name] = (outer, K, inner, torch.from_numpy(p).to(dev()), torch.from_numpy(label).to(dev()),
                     torch.full((outer, inner), -1.0, dtype=torch.float32, device=dev()))
    return out


@pytest.mark.parametrize('normalize', [0, 1])
@pytest.mark.parametrize('path', ['rows', 'strided'])
@pytest.mark.parametrize('S', SCALES)
def test_softmax_gradient_with_the_scale_on_the_device(softmax_cases, S, path, normalize):
    hip = _hip()
    outer, K, inner, p, label, all_ignored = softmax_cases[path]
    gs = 0.75
    n = outer * K * inner
    labels = [label] + ([all_ignored] if normalize else [])         # (count 0 becomes 1)
    for lab in labels:
        cnt_a, cnt_b = (torch.zeros(4, dtype=torch.int32, device=dev()) for _ in range(2))
        buf_a, ga = _padded(n)
        buf_b, gb = _padded(n)
        hip.call('sn_softmax_output_bwd', p, lab, ga, outer, K, inner, -1.0, 1, float(np.float32(gs) * np.float32(S)), normalize, cnt_a,
                 hip.stream())
        ls = _ls(S)
        hip.call('sn_softmax_output_bwd_scaled', p, lab, gb, outer, K, inner, -1.0, 1, gs, normalize, cnt_b, ls, hip.stream())
        assert torch.equal(buf_a.view(torch.int32), buf_b.view(torch.int32)), (S, path, normalize)
        assert (buf_b[:8] == -7.5).all() and (buf_b[-8:] == -7.5).all()
        assert torch.equal(cnt_a, cnt_b) and torch.equal(ls, _ls(S))
        if lab is label:
            assert ga.abs().max() > 0
            # and it is the gradient: scale * grad_scale / valid * (p - onehot) where the label is not ignored
            valid = int((lab != -1).sum()) if normalize else 1
            mul = np.float32(np.float32(gs) * np.float32(S)) / np.float32(max(valid, 1))
            l = lab.cpu().numpy()
            onehot = (np.arange(K)[None, :, None] == l[:, None, :]).astype(np.float32)
            want = np.where(l[:, None, :] == -1, np.float32(0), mul * (p.cpu().numpy() - onehot)).astype(np.float32)
            assert np.array_equal(ga.cpu().numpy().reshape(outer, K, inner), want)
        else:
            assert not ga.any() and int(cnt_b[0]) == 0


@pytest.mark.parametrize('S', SCALES)
def test_fill_with_the_scale_on_the_device(S):
    hip = _hip()
    value = 4.6875 / 3
    for n in (1, 255, 256, 257, 1025):
        buf_a, a = _padded(n)
        buf_b, b = _padded(n)
        hip.call('sn_ew_f32', None, None, a, n, 4, float(np.float32(value) * np.float32(S)), hip.stream())
        hip.call('sn_fill_scaled_f32', b, n, value, _ls(S), hip.stream())
        assert torch.equal(buf_a.view(torch.int32), buf_b.view(torch.int32)), (S, n)
        assert (buf_b[:8] == -7.5).all() and (buf_b[-8:] == -7.5).all() and (b == float(np.float32(value) * np.float32(S))).all()


# ------------------------------------------------------------------------------------------------
# 2. sn_grad_guard_scaled
# ------------------------------------------------------------------------------------------------
N_ARENA = 3 * 4096 + 5


class ScaledGuard(object):
    """device state, scaler state and workspace; the restatement runs beside them from its OWN state (whole trajectories compare)"""

    def __init__(self, init_scale, rescale=-0.5, **policy):
        hip = _hip()
        self.policy = dict(growth_interval=3, growth_factor=2.0, backoff_factor=0.5, min_scale=1.0, max_scale=2.0 ** 24)
        self.policy.update(policy)
        self.rescale = rescale
        self.hyper = torch.tensor([0.01, 1e-4, 0.9, rescale], dtype=torch.float32, device=dev())
        self.state = torch.zeros(8, dtype=torch.float64, device=dev())
        self.ls = _ls(init_scale)
        self.ws = torch.empty(max(int(hip.query('sn_grad_guard_workspace_bytes', N_ARENA, 0)), 256), dtype=torch.uint8, device=dev())
        self.want_state, self.want_ls = np.zeros(8), ref.new_ls(init_scale)

    def run(self, view, clip):
        hip = _hip()
        p = self.policy
        hip.call('sn_grad_guard_scaled', view, view.numel(), self.hyper, float(clip), 0, p['growth_interval'], p['growth_factor'],
                 p['backoff_factor'], p['min_scale'], p['max_scale'], self.ws, self.state, self.ls, hip.stream())
        self.want_state, self.want_ls = ref.guard_scaled(view.cpu().numpy(), self.rescale, clip, self.want_state, self.want_ls, **p)
        return self.state.cpu().numpy(), self.ls.cpu().numpy()


def _arena(vals, off):
    buf = torch.full((vals.size + off + 8,), float('nan'), dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + vals.size]
    view.copy_(torch.from_numpy(vals))
    return view


@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_guard_scaled_trajectory_against_the_restatement(off):
    """sixteen consecutive calls on integer gradients (every summation order exact), growth_interval 3, inf / NaN planted at steps
    2, 3 and 9: the guard's and the scaler's eight doubles equal the restatement's bit for bit after every call"""
    rs = np.random.RandomState(31 + off)
    g = ScaledGuard(2.0 ** 7)
    poison = {2: [(0, np.inf)], 3: [(N_ARENA - 1, np.nan), (4097, -np.inf)], 9: [(N_ARENA // 2, np.nan)]}
    scales, clipped = [], 0
    for step in range(16):
        vals = rs.randint(-8, 9, N_ARENA).astype(np.float32)
        for pos, v in poison.get(step, ()):
            vals[pos] = v
        clip = (0.0, 1.0)[step & 1]
        state, ls = g.run(_arena(vals, off), clip)
        assert np.array_equal(state, g.want_state), (step, state, g.want_state)
        assert np.array_equal(ls, g.want_ls), (step, ls, g.want_ls)
        S = ls[1]
        assert state[0] == np.sqrt(state[7]) * 0.5 / S and state[2] == (1.0 if step in poison else 0.0)
        assert state[3] == len(poison.get(step, ())) and state[4] == step + 1
        if clip > 0 and state[0] > 1.0:
            c = 1.0 / (state[0] + 1e-6)
            assert c < 1.0 and state[1] == c / S
            clipped += 1
        else:
            assert state[1] == 1.0 / S
        scales.append(ls[0])
    assert clipped >= 4
    assert scales == [128, 128, 64, 32, 32, 32, 64, 64, 64, 32, 32, 32, 64, 64, 64, 128]
    assert ls.tolist() == [128.0, 64.0, 0.0, 3.0, 3.0, 0.0, 0.0, 0.0]


def test_guard_scaled_clamps():
    rs = np.random.RandomState(5)
    clean = rs.randint(-8, 9, N_ARENA).astype(np.float32)
    bad = clean.copy()
    bad[77] = np.inf
    g = ScaledGuard(2.0 ** 10, growth_interval=1, max_scale=2.0 ** 10)
    for k in (1, 2):
        state, ls = g.run(_arena(clean, 0), 0.0)
        assert np.array_equal(ls, g.want_ls) and np.array_equal(state, g.want_state)
        assert ls.tolist() == [1024.0, 1024.0, 0.0, 0.0, 0.0, float(k), 0.0, 0.0]
    g = ScaledGuard(2.0 ** -2, min_scale=2.0 ** -2, max_scale=1.0)
    state, ls = g.run(_arena(bad, 1), 0.0)
    assert np.array_equal(ls, g.want_ls) and np.array_equal(state, g.want_state)
    assert ls.tolist() == [0.25, 0.25, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0] and state[2] == 1.0
    # growth_interval 0 never grows; a back-off of 1/4 that min_scale cuts short lowers the scale AND counts as held
    g = ScaledGuard(2.0, growth_interval=0, backoff_factor=0.25)
    for _ in range(3):
        state, ls = g.run(_arena(clean, 2), 0.0)
    assert ls.tolist() == [2.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    state, ls = g.run(_arena(bad, 2), 0.0)
    assert np.array_equal(ls, g.want_ls) and ls.tolist() == [1.0, 2.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------
# 3. unscaling inside the guarded update is exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', [2.0 ** 7, 2.0 ** 15])
def test_unscaling_in_the_guarded_update_is_exact(S):
    """coef = 0.5 / S on gradients g * S against coef = 0.5 on g (|g| <= 8: g * S is finite and exact): the same bits"""
    from test_gpu_grad_guard import SLICES, _guarded, _state, _update_data
    n = 100003
    w, g, m, h = _update_data(n)
    gS = (g * np.float32(S)).astype(np.float32)
    assert np.isfinite(gS).all() and np.array_equal(gS / np.float32(S), g)
    for off, cnt in SLICES(n):
        w1, _, m1, h1, _ = _guarded(w, g, m, h, off, cnt, 0.0, _state(coef=0.5))
        w2, _, m2, h2, _ = _guarded(w, gS, m, h, off, cnt, 0.0, _state(coef=0.5 / S))
        assert torch.equal(w1.view(torch.int32), w2.view(torch.int32)) and torch.equal(m1.view(torch.int32), m2.view(torch.int32)), (off, cnt)
        assert torch.equal(h1.view(torch.int16), h2.view(torch.int16)), (off, cnt)
        assert not torch.equal(w1, torch.from_numpy(w).to(dev()))


# ------------------------------------------------------------------------------------------------
# 4. sn_aux_shadow
# ------------------------------------------------------------------------------------------------
def test_aux_shadow_saves_and_restores_on_skip_only():
    hip = _hip()
    lengths = (1, 63, 64, 65, 2048, 2049, 5)
    rs = np.random.RandomState(9)
    offs, o = [], 1
    for n in lengths:
        offs.append(o)                      # odd float offsets, at least three floats of padding between the vectors
        o += n + 3
        o += 1 - (o & 1)
    size = o + 8
    host = np.full(size, -3.25, np.float32)
    for n, a in zip(lengths, offs):
        assert a & 1
        host[a:a + n] = rs.standard_normal(n).astype(np.float32)
    host[offs[1]] = np.float32(np.nan)                      # (bits, not values: a NaN is saved and restored like anything else)
    buf = torch.from_numpy(host.copy()).to(dev())
    total = sum(lengths)
    rec = np.zeros(len(lengths), dtype=np.dtype([('ptr', '<u8'), ('off', '<i4'), ('n', '<i4')]))
    so = 0
    for k, (n, a) in enumerate(zip(lengths, offs)):
        rec[k] = (buf.data_ptr() + 4 * a, so, n)
        so += n
    table = torch.from_numpy(rec.view(np.uint8).copy()).to(dev())
    shadow = torch.full((total + 16,), 9.5, dtype=torch.float32, device=dev())
    state = lambda skip: torch.tensor([0, 1, skip, 0, 0, 0, 0, 0], dtype=torch.float64, device=dev())
    hip.call('sn_aux_shadow', table, len(lengths), shadow, 0, None, hip.stream())
    want_shadow = np.concatenate([host[a:a + n] for n, a in zip(lengths, offs)])
    assert np.array_equal(shadow[:total].cpu().numpy().view(np.int32), want_shadow.view(np.int32))
    assert (shadow[total:] == 9.5).all() and np.array_equal(buf.cpu().numpy().view(np.int32), host.view(np.int32))
    # the forward overwrites the sources, some with NaN
    over = host.copy()
    for k, (n, a) in enumerate(zip(lengths, offs)):
        over[a:a + n] = np.nan if k % 2 == 0 else rs.standard_normal(n).astype(np.float32)
    buf.copy_(torch.from_numpy(over))
    hip.call('sn_aux_shadow', table, len(lengths), shadow, 1, state(0.0), hip.stream())
    assert np.array_equal(buf.cpu().numpy().view(np.int32), over.view(np.int32))           # not skipped: the new values stay
    hip.call('sn_aux_shadow', table, len(lengths), shadow, 1, state(1.0), hip.stream())
    assert np.array_equal(buf.cpu().numpy().view(np.int32), host.view(np.int32))           # skipped: the saved bits, padding untouched
    assert (shadow[total:] == 9.5).all() and np.array_equal(shadow[:total].cpu().numpy().view(np.int32), want_shadow.view(np.int32))
    # and it agrees with the restatement's shadow
    vecs = [over[a:a + n].copy() for n, a in zip(lengths, offs)]
    sh = ref.Shadow([host[a:a + n].copy() for n, a in zip(lengths, offs)])
    sh.save()
    sh.vectors = vecs
    sh.restore([0, 0, 1.0])
    assert all(np.array_equal(v.view(np.int32), host[a:a + n].view(np.int32)) for v, n, a in zip(vecs, lengths, offs))


# ------------------------------------------------------------------------------------------------
# 5. steps of a small graph, eager and captured
# ------------------------------------------------------------------------------------------------
A_, B_, S_ = 3, 2, 64
F_ = S_ // 8
SHAPES = dict(data=(B_, 3, S_, S_), label=(B_, A_ * F_ * F_), bbox_target=(B_, 4 * A_, F_, F_), bbox_weight=(B_, 4 * A_, F_, F_))
SGD = dict(lr=1e-4, wd=1e-3, momentum=0.9)
INIT = 128.0


def _mini_graph(mx, A=3, gs=100.0):
    """tests/test_gpu_engine.py::_mini_graph with the loss scale `gs` of its two grad_scale attributes as a parameter: fp16 storage
    behind the stem, batch-statistics BatchNorm (momentum 0.9) in the two bottleneck units"""
    data = mx.sym.Variable('data')
    label, target, weight = mx.sym.Variable('label'), mx.sym.Variable('bbox_target'), mx.sym.Variable('bbox_weight')
    x = mx.sym.BatchNorm(data=data, name='bn_data', fix_gamma=True, eps=2e-5, use_global_stats=True)
    x = mx.sym.Convolution(data=x, name='conv0', num_filter=64, kernel=(7, 7), stride=(2, 2), pad=(3, 3), no_bias=True)
    x = mx.sym.Cast(data=x, dtype=np.float16)
    x = mx.sym.BatchNorm(data=x, name='bn0', fix_gamma=False, eps=2e-5, use_global_stats=True)
    x = mx.sym.Activation(data=x, act_type='relu', name='relu0')
    x = mx.sym.Pooling(data=x, kernel=(3, 3), stride=(2, 2), pad=(1, 1), pool_type='max')

    def unit(x, nf, stride, match, name):
        a1 = mx.sym.Activation(data=mx.sym.BatchNorm(data=x, name=name + '_bn1', fix_gamma=False, eps=2e-5, momentum=0.9),
                               act_type='relu', name=name + '_relu1')
        c1 = mx.sym.Convolution(data=a1, name=name + '_conv1', num_filter=nf // 4, kernel=(1, 1), no_bias=True)
        a2 = mx.sym.Activation(data=mx.sym.BatchNorm(data=c1, name=name + '_bn2', fix_gamma=False, eps=2e-5, momentum=0.9),
                               act_type='relu', name=name + '_relu2')
        c2 = mx.sym.Convolution(data=a2, name=name + '_conv2', num_filter=nf // 4, kernel=(3, 3), stride=(stride, stride),
                                pad=(1, 1), no_bias=True)
        a3 = mx.sym.Activation(data=mx.sym.BatchNorm(data=c2, name=name + '_bn3', fix_gamma=False, eps=2e-5, momentum=0.9),
                               act_type='relu', name=name + '_relu3')
        c3 = mx.sym.Convolution(data=a3, name=name + '_conv3', num_filter=nf, kernel=(1, 1), no_bias=True)
        sc = x if match else mx.sym.Convolution(data=a1, name=name + '_sc', num_filter=nf, kernel=(1, 1),
                                                stride=(stride, stride), no_bias=True)
        return c3 + sc

    u1 = unit(x, 128, 2, False, 'stage2_unit1')
    u2 = unit(u1, 128, 1, True, 'stage2_unit2')
    cat = mx.sym.Cast(data=mx.sym.Concat(u1, u2, name='cat4'), dtype=np.float32)
    r = mx.sym.Activation(data=mx.sym.Convolution(data=cat, kernel=(3, 3), pad=(1, 1), num_filter=64, name='rpn_conv_3x3'),
                          act_type='relu', name='rpn_relu')
    cls = mx.sym.Convolution(data=r, kernel=(1, 1), num_filter=2 * A, name='rpn_cls_score')
    box = mx.sym.Convolution(data=r, kernel=(1, 1), num_filter=4 * A, name='rpn_bbox_pred')
    cls_r = mx.sym.Reshape(data=cls, shape=(0, 2, -1, 0), name='rpn_cls_score_reshape')
    prob = mx.sym.SoftmaxOutput(data=cls_r, label=label, multi_output=True, normalization='valid', use_ignore=True,
                                ignore_label=-1, name='rpn_cls_prob', grad_scale=gs)
    l1 = weight * mx.sym.smooth_l1(name='rpn_bbox_loss_', scalar=1.0, data=(box - target))
    loss = mx.sym.MakeLoss(name='rpn_bbox_loss', data=l1, grad_scale=3 * gs / 64.0)
    return mx.sym.Group([prob, loss])


@pytest.fixture(scope='module')
def problem():
    """parameters and eight batches of the small graph, made once and never changed"""
    import sniper_amd.mx as mx
    rs = np.random.RandomState(5)
    sym = _mini_graph(mx, A_)
    args, _, auxs = sym.infer_shape(**SHAPES)
    P, AUX = {}, {}
    for name, shp in zip(sym.list_arguments(), args):
        if name not in SHAPES:
            P[name] = rs.uniform(0.5, 1.5, shp).astype(np.float32) if name.endswith('_gamma') else \
                (rs.standard_normal(shp) * (0.1 if len(shp) == 1 else np.sqrt(2.0 / np.prod(shp[1:])))).astype(np.float32)
    for name, shp in zip(sym.list_auxiliary_states(), auxs):
        AUX[name] = rs.uniform(0.5, 1.5, shp).astype(np.float32)
    feeds = [dict(data=(rs.standard_normal((B_, 3, S_, S_)) * 2).astype(np.float32),
                  label=rs.choice([-1, 0, 1], size=(B_, A_ * F_ * F_), p=[0.5, 0.3, 0.2]).astype(np.float32),
                  bbox_target=rs.standard_normal((B_, 4 * A_, F_, F_)).astype(np.float32),
                  bbox_weight=(rs.uniform(size=(B_, 4 * A_, F_, F_)) < 0.2).astype(np.float32)) for _ in range(8)]
    return P, AUX, feeds


def _overflowing(feed):
    bad = dict(feed)
    bad['data'] = feed['data'].copy()
    bad['data'][0, 1, 17, 23] = np.inf
    return bad


def _executor(problem, gs=100.0):
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    from sniper_amd.mx import symbol
    symbol._counter().clear()
    sym = _mini_graph(mx, A_, gs)
    fixed = [n for n in sym.list_arguments() if any(p in n for p in ('conv0', 'bn0', 'bn_data'))]
    ex = Executor(sym, SHAPES, True, fixed)
    ex.set_params(problem[0], problem[1])
    return ex


def _params(ex):
    out = {'master': ex.arena_master.clone(), 'mom': ex.arena_mom.clone(), 'w16': ex.arena_w16.clone().view(torch.int16)}
    for k, p in ex.params.items():
        if p.trainable and p.wT16 is not None:
            out['wT16.' + k] = p.wT16.clone().view(torch.int16)
    return out


def _aux(ex):
    return {'aux.' + k: t.clone().view(torch.int32) for k, t in ex.aux.items()}


def _differ(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def _lstate(ex):
    return dict(zip(ref.LS_KEYS, ex.loss_scale['state'].cpu().tolist()))


@pytest.fixture(params=['eager', 'captured'])
def mode(request, monkeypatch):
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', '1' if request.param == 'captured' else '0')
    return request.param


def test_fixed_dynamic_scale_is_the_static_scale(mode, problem):
    """5a: a static graph with gs = 100 * 128, lr / 128, wd * 128 against gs = 100 with set_loss_scale(128, growth_interval=0) and the
    true lr / wd, four steps (two eager, the capture, a replay): the gradient arena bit-equal after every forward_backward, the
    moving statistics bit-equal, masters / momentum / fp16 copies within the active-path bound after every update"""
    a, b = _executor(problem, 100.0 * INIT), _executor(problem, 100.0)
    b.set_loss_scale(INIT, growth_interval=0)
    assert b.guard is not None and b.guard['skip_nonfinite'] == 1 and b.loss_scale['n_aux'] == 12
    for i, feed in enumerate(problem[2][:4]):
        a.forward_backward(feed)
        b.forward_backward(feed)
        same = torch.equal(a.arena_grad.view(torch.int32), b.arena_grad.view(torch.int32))
        print('step %d: arena_grad bit-equal %s, max |a - b| %.3g of max |a| %.3g' % (
            i, same, float((a.arena_grad - b.arena_grad).abs().max()), float(a.arena_grad.abs().max())))
        assert same, i
        assert _differ(_aux(a), _aux(b)) == [], i
        a.update(lr=SGD['lr'] / INIT, wd=SGD['wd'] * INIT, momentum=SGD['momentum'])
        b.update(**SGD)
        pa, pb = _params(a), _params(b)
        for k in ('master', 'mom'):
            print('step %d: %s max |a - b| %.3g' % (i, k, float((pa[k] - pb[k]).abs().max())))
            assert torch.allclose(pb[k], pa[k], rtol=RTOL, atol=ATOL), (i, k)
        h_a, h_b = a.arena_w16.float(), b.arena_w16.float()
        print('step %d: w16 max |a - b| %.3g' % (i, float((h_a - h_b).abs().max())))
        assert torch.allclose(h_b, h_a, rtol=RTOL, atol=ATOL), i
    assert (b._graph_up is not None) == (b._graph_fb is not None) == (mode == 'captured')
    st = _lstate(b)
    assert st['scale'] == INIT and st['scale_used'] == INIT and st['clean'] == 4 and st['growths'] == 0 and st['backoffs'] == 0
    assert b.guard['state'].cpu()[4] == 4 and b.guard['state'].cpu()[5] == 0


@pytest.mark.parametrize('restore_aux', [True, False])
def test_forward_overflow_is_a_no_op(mode, problem, restore_aux):
    """5b: four clean steps, then a batch whose data holds one inf: masters, momentum, fp16 and transposed copies AND every moving
    statistic are bit-equal to before the step; the scale is halved.  A clean step afterwards moves the parameters and all
    statistics are finite.  restore_aux=False: the same batch leaves non-finite statistics (the test sees the effect)."""
    ex = _executor(problem)
    ex.set_loss_scale(INIT, restore_aux=restore_aux)
    feeds = problem[2]
    for feed in feeds[:4]:
        ex.forward_backward(feed)
        ex.update(**SGD)
    assert (ex._graph_up is not None) == (ex._graph_fb is not None) == (mode == 'captured')
    assert _lstate(ex)['clean'] == 4 and _lstate(ex)['scale'] == INIT
    before, aux_before = _params(ex), _aux(ex)
    assert all(torch.isfinite(t).all() for t in ex.aux.values())
    ex.forward_backward(_overflowing(feeds[4]))
    ex.update(**SGD)
    assert _differ(before, _params(ex)) == []
    st = _lstate(ex)
    assert st['scale'] == INIT / 2 and st['scale_used'] == INIT and st['clean'] == 0 and st['backoffs'] == 1 and st['growths'] == 0
    g = ex.guard['state'].cpu().tolist()
    assert g[2] == 1.0 and g[3] > 0 and g[5] == 1.0
    if not restore_aux:
        assert ex.loss_scale['n_aux'] == 0
        assert any(not torch.isfinite(t).all() for t in ex.aux.values())
        return
    assert _differ(aux_before, _aux(ex)) == []
    ex.forward_backward(feeds[5])
    ex.update(**SGD)
    moved = _differ(before, _params(ex))
    assert 'master' in moved and 'mom' in moved and 'w16' in moved
    assert all(torch.isfinite(t).all() for t in ex.aux.values()) and _differ(aux_before, _aux(ex)) != []
    assert torch.isfinite(ex.arena_master).all() and torch.isfinite(ex.arena_mom).all()
    st = _lstate(ex)
    assert st['scale'] == INIT / 2 and st['scale_used'] == INIT / 2 and st['clean'] == 1


def test_growth_after_clean_steps(mode, problem):
    """5c: growth_interval 3: six clean steps double the scale twice, and the gradients of step 4 carry the doubled scale"""
    ex = _executor(problem)
    ex.set_loss_scale(INIT, growth_interval=3)
    used = []
    for feed in problem[2][:6]:
        ex.forward_backward(feed)
        ex.update(**SGD)
        used.append(_lstate(ex)['scale_used'])
    assert used == [INIT] * 3 + [2 * INIT] * 3
    st = _lstate(ex)
    assert st['scale'] == 4 * INIT and st['growths'] == 2 and st['clean'] == 0 and st['backoffs'] == 0
    assert ex.guard['state'].cpu()[5] == 0 and torch.isfinite(ex.arena_master).all()
    assert (ex._graph_fb is not None) == (mode == 'captured')


def test_too_large_a_start_finds_its_level(mode, problem):
    """5d: init_scale 2^30 overflows the fp16 activations' gradients; every skipped step halves the scale until a step goes through
    (31 steps at most: 2^30 reaches 2^0 in 30 back-offs)"""
    ex = _executor(problem)
    ex.set_loss_scale(2.0 ** 30, min_scale=1.0, max_scale=2.0 ** 30)
    before = _params(ex)
    aux_before = _aux(ex)
    feeds = problem[2]
    done = None
    for i in range(31):
        ex.forward_backward(feeds[i % len(feeds)])
        ex.update(**SGD)
        if ex.guard['state'].cpu()[2] == 0.0:
            done = i
            break
        assert _differ(before, _params(ex)) == [] and _differ(aux_before, _aux(ex)) == [], i
    assert done is not None
    st = _lstate(ex)
    print('first step that went through: %d, at scale %g' % (done, st['scale_used']))
    assert done > 0, 'the small graph does not overflow at 2^30'
    assert st['backoffs'] == np.log2(2.0 ** 30 / st['scale_used']) == done and st['clean'] == 1
    assert torch.isfinite(ex.arena_master).all() and all(torch.isfinite(t).all() for t in ex.aux.values())
    assert 'master' in _differ(before, _params(ex))


def test_module_reports_back_off_and_growth(problem, caplog):
    """Module.init_optimizer(dynamic_loss_scale=...): the lagged snapshot carries the scaler's state; a back-off is logged once at
    warning level with the old and the new scale, a growth at info level; synchronised so that every snapshot has landed before the
    next update inspects it"""
    import logging
    import sniper_amd.mx as mx
    P, AUX, feeds = problem
    sym = _mini_graph(mx, A_)
    labels = ['label', 'bbox_target', 'bbox_weight']
    fixed = [n for n in sym.list_arguments() if any(p in n for p in ('conv0', 'bn0', 'bn_data'))]
    mod = mx.mod.Module(sym, data_names=['data'], label_names=labels, context=[mx.gpu(0)], fixed_param_names=fixed)
    mod.bind(data_shapes=[('data', SHAPES['data'])], label_shapes=[(k, SHAPES[k]) for k in labels], for_training=True)
    mod.init_params(arg_params=P, aux_params=AUX)
    assert mod.loss_scale_state() is None
    mod.init_optimizer(optimizer='sgd', optimizer_params={'learning_rate': 1e-4, 'momentum': 0.9, 'wd': 1e-3,
                                                          'dynamic_loss_scale': {'init_scale': INIT, 'growth_interval': 2}})
    assert mod.loss_scale_state()['scale'] == INIT and mod.loss_scale_state(wait=False) is None
    assert mod.grad_guard_state()['steps'] == 0

    def step(feed):
        mod.forward_backward(mx.io.DataBatch(data=[feed['data']], label=[feed[k] for k in labels]))
        mod.update()
        torch.cuda.synchronize()
    msgs = lambda: [(r.levelno, r.getMessage()) for r in caplog.records if r.getMessage().startswith('loss scale')]
    with caplog.at_level(logging.INFO):
        step(feeds[0])
        before = mod.exe.arena_master.clone()
        step(_overflowing(feeds[1]))
        assert msgs() == [] and torch.equal(before, mod.exe.arena_master)
        lag = mod.loss_scale_state(wait=False)
        assert lag['scale'] == INIT / 2 and lag['scale_used'] == INIT and lag['backoffs'] == 1 and lag['clean'] == 0
        assert mod.grad_guard_state(wait=False)['skipped_last'] is True
        step(feeds[2])
        got = msgs()
        assert len(got) == 1 and got[0][0] == logging.WARNING and 'step 2 skipped' in got[0][1] and '128 -> 64' in got[0][1]
        step(feeds[3])                       # the second clean step at 64: back to 128
        step(feeds[4])
        got = msgs()
        assert len(got) == 2 and got[1][0] == logging.INFO and 'step 4' in got[1][1] and '64 -> 128' in got[1][1]
    st = mod.loss_scale_state()
    assert st == dict(scale=INIT, scale_used=INIT, clean=1, growths=1, backoffs=1, held_max=0, held_min=0)
    assert mod.grad_guard_state()['skipped'] == 1 and not torch.equal(before, mod.exe.arena_master)


def test_trainer_with_dynamic_loss_scale():
    """5e: the R101 step with the scale on the device: three steps, finite outputs, the scale still where it started (128: the power
    of two nearest to the config's static 100), three guarded steps"""
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=2, n_images=4, seed=0, dynamic_loss_scale=True)
    ex = tr.mod.exe
    assert ex.loss_scale is not None and ex.guard is not None and ex.loss_scale['n_aux'] > 0
    assert tr.mod.opt['lr'] == tr.cfg.TRAIN.lr and tr.mod.opt['wd'] == tr.cfg.TRAIN.wd
    before = ex.arena_master.clone()
    for _ in range(3):
        outs = tr.step()
        for o in outs:
            assert np.isfinite(o.asnumpy()).all()
    ls, st = tr.mod.loss_scale_state(), tr.mod.grad_guard_state()
    print('scaler %r\nguard %r' % (ls, st))
    assert ls['scale'] == 128 and ls['scale_used'] == 128 and ls['clean'] == 3 and ls['backoffs'] == 0
    assert sorted(ls) == sorted(('scale', 'scale_used', 'clean', 'growths', 'backoffs', 'held_max', 'held_min'))
    assert st['steps'] == 3 and st['skipped'] == 0 and np.isfinite(st['norm']) and st['norm'] > 0
    assert st['coef'] == 1.0 / 128
    assert torch.isfinite(ex.arena_master).all() and not torch.equal(before, ex.arena_master)
