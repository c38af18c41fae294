"""-m gpu: the gradient guard -- sn_grad_guard against its numpy restatement (tests/grad_guard_ref.py) with exact sums at every edge of
the peel / body / tail split and of the grid-stride loop, non-finite elements at every position, the guarded update on its three
paths (skipped: nothing written; inactive: the bits of sn_sgd_mom_update_dev; active: the restatement), then the optimizer pass of a
small graph, eager and captured, a Module that gives up after consecutive skipped steps, and the R101 Trainer."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import grad_guard_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-7          # one-ulp contraction differences (tests/test_gpu_nn_ops.py::test_sgd_and_weight_transpose)
SLICES = lambda n: ((0, n), (3, n - 5), (1, 2), (2, 65541), (4, 64))


def _hip():
    from sniper_amd import hip
    return hip


def _limits():
    out = (ctypes.c_int32 * 4)()
    _hip().lib().call('sn_grad_guard_limits', out)
    return tuple(int(v) for v in out)


class Guard(object):
    """one device state + workspace, and the restatement's state beside it"""

    def __init__(self, rescale=-0.5):
        hip = _hip()
        _, _, cap, nstate = _limits()
        assert nstate == 8
        self.hyper = torch.tensor([0.01, 1e-4, 0.9, rescale], dtype=torch.float32, device=dev())
        self.rescale = rescale
        self.state = torch.zeros(8, dtype=torch.float64, device=dev())
        self.ws = torch.empty(max(int(hip.query('sn_grad_guard_workspace_bytes', 1 << 40, 0)), 16 * 65535), dtype=torch.uint8, device=dev())
        self.want = np.zeros(8)

    def run(self, view, clip, skip, max_blocks=0):
        """-> (device state, restated state) after one call over the device view; the restatement continues from the DEVICE's state"""
        hip = _hip()
        before = self.state.cpu().numpy()
        hip.call('sn_grad_guard', view, view.numel(), self.hyper, float(clip), int(skip), int(max_blocks), self.ws, self.state, hip.stream())
        got = self.state.cpu().numpy()
        return got, ref.guard(view.cpu().numpy(), self.rescale, clip, skip, before)


def _placed(values, off, pad=8):
    """values at `off` floats behind a 16-byte boundary; everything around them is NaN (a read outside [0, n) would be counted)"""
    buf = torch.full((values.size + off + pad,), float('nan'), dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + values.size]
    view.copy_(torch.from_numpy(values))
    return view


def _exact_sizes():
    T, E, _, _ = _limits()
    S = T * E
    base = [1, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1, S - 1, S, S + 1, 2 * S + 1]
    cases = [(n, mb) for mb in (0, 1, 2, 3) for n in base]
    cases += [(mb * S + d, mb) for mb in (1, 2, 3) for d in (-1, 0, 1)]
    return cases


@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_exact_sums_at_every_edge(off):
    """integer gradients in [-8, 8]: every partial sum is an integer far below 2^53, so ANY order of summation is exact and the
    state equals the restatement bit for bit -- sizes around the wave, the block, the block's span per trip and the grid-stride wrap
    (max_blocks 1, 2, 3), each at this offset from a 16-byte boundary; the counters advance by one per call."""
    rs = np.random.RandomState(17 + off)
    g = Guard()
    calls = 0
    for n, mb in _exact_sizes():
        vals = rs.randint(-8, 9, n).astype(np.float32)
        view = _placed(vals, off)
        clip = (0.0, 3.0, 1e9)[calls % 3]
        got, want = g.run(view, clip, True, mb)
        calls += 1
        assert got[7] == float(np.sum(vals.astype(np.float64) ** 2)), (n, mb, off)
        assert np.array_equal(got, want), (n, mb, off, got, want)
        assert got[4] == calls and got[3] == 0 and got[2] == 0 and got[5] == 0
        if clip == 3.0 and got[0] > 3.0:
            assert got[1] < 1.0
    assert calls == len(_exact_sizes())


def test_random_data_within_the_summation_bound_and_reproducible():
    """n = 100003 standard normal: sumsq within n * 2^-53 relative of numpy's fp64 sum -- the bound for ANY order of summing n
    non-negative terms (each addition adds at most 2^-53 relative, at most n - 1 additions lie above a term); two calls give the
    same bits in everything but the counters."""
    n = 100003
    vals = np.random.RandomState(2).standard_normal(n).astype(np.float32)
    view = _placed(vals, 1)
    g = Guard(rescale=0.75)
    a, want = g.run(view, 10.0, True)
    b, _ = g.run(view, 10.0, True)
    print('sumsq device %.17g numpy %.17g rel %.3g bound %.3g' % (a[7], want[7], abs(a[7] - want[7]) / want[7], n * 2.0 ** -53))
    assert abs(a[7] - want[7]) <= n * 2.0 ** -53 * want[7]
    assert abs(a[0] - want[0]) <= n * 2.0 ** -53 * want[0] and a[0] == np.sqrt(a[7]) * 0.75
    assert a[1] == min(1.0, 10.0 / (a[0] + 1e-6)) and a[1] < 1.0
    keep = [0, 1, 2, 3, 7]
    assert a[keep].tobytes() == b[keep].tobytes() and (a[4], b[4]) == (1.0, 2.0)
    for mb in (1, 7):                   # another grid: another order, the same bound
        c, _ = g.run(view, 10.0, True, mb)
        assert abs(c[7] - want[7]) <= n * 2.0 ** -53 * want[7]


def _poison_positions():
    """floats at 1 behind a 16-byte boundary, n = 2 spans + 9: a peeled head of 3, a four-wide body, a tail of 2"""
    T, E, _, _ = _limits()
    n = 2 * T * E + 9
    return n, {'first': 0, 'head': 2, 'body': T * E + 5, 'tail': n - 2, 'last': n - 1}


@pytest.mark.parametrize('skip', [True, False])
def test_non_finite_elements_are_counted_and_left_out(skip):
    n, pos = _poison_positions()
    rs = np.random.RandomState(23)
    clean = rs.randint(-8, 9, n).astype(np.float32)
    g = Guard(rescale=1.0)
    cases = [[(p, v)] for p in pos.values() for v in (np.inf, -np.inf, np.nan)]
    cases.append(list(zip(pos.values(), (np.inf, np.nan, -np.inf, np.nan, np.inf))))
    cases.append([(pos['body'], np.nan), (pos['body'] + 1, np.inf), (pos['last'], -np.inf)])
    for case in cases:
        vals = clean.copy()
        for p, v in case:
            vals[p] = v
        got, want = g.run(_placed(vals, 1), 0.0, skip)
        rest = np.delete(clean, [p for p, _ in case]).astype(np.float64)
        assert got[3] == len(case) and got[7] == float(np.sum(rest * rest)), case
        assert got[2] == (1.0 if skip else 0.0) and np.array_equal(got, want), (case, got, want)
        g.run(_placed(clean, 1), 0.0, skip)          # a clean call in between: every poisoned call is the first of a run
        assert g.state.cpu()[6] == 0
    # consecutive: up over three poisoned calls, back to 0 on a clean one
    g = Guard(rescale=1.0)
    bad = clean.copy()
    bad[pos['body']] = np.nan
    seen = [g.run(_placed(v, 1), 0.0, skip)[0] for v in (bad, bad, bad, clean, bad)]
    assert [s[6] for s in seen] == ([1, 2, 3, 0, 1] if skip else [0] * 5)
    assert [s[5] for s in seen] == ([1, 2, 3, 3, 4] if skip else [0] * 5) and [s[4] for s in seen] == [1, 2, 3, 4, 5]
    assert [s[3] for s in seen] == [1, 1, 1, 0, 1]


def _update_data(n, seed=6):
    """|w| <= 1, |m| <= 0.5, |g| <= 8 with lr <= 0.02: |new m| < 1 and |new w| < 2, so a one-ulp difference of a contracted
    multiply-add (2^-24 on m, carried into w) stays inside atol = 1e-7 -- the bound is for such differences, not for cancellation"""
    rs = np.random.RandomState(seed)
    w = rs.uniform(-1, 1, n).astype(np.float32)
    g = (rs.standard_normal(n) * 2).clip(-8, 8).astype(np.float32)
    g[::7] = np.where(rs.uniform(size=g[::7].size) < 0.5, 1.0, -1.0)        # rescale 0.5 * 1.0: exactly on clip_gradient = 0.5
    m = rs.uniform(-0.5, 0.5, n).astype(np.float32)
    h = rs.standard_normal(n).astype(np.float16)
    return w, g, m, h


def _state(coef=1.0, skip=0.0):
    return torch.tensor([1.0, coef, skip, 3.0 * skip, 5.0, skip, skip, 1.0], dtype=torch.float64, device=dev())


HYPER = (0.01, 0.001, 0.9, 0.5)


def _guarded(w, g, m, h, off, cnt, clip, state):
    hip = _hip()
    td = lambda z: torch.from_numpy(z.copy()).to(dev())
    w1, g1, m1, h1 = td(w), td(g), td(m), td(h)
    hyper = torch.tensor(HYPER, dtype=torch.float32, device=dev())
    hip.call('sn_sgd_mom_update_guarded_dev', w1[off:], g1[off:], m1[off:], h1[off:], cnt, hyper, 2.0, 0.5, float(clip), state, hip.stream())
    return w1, g1, m1, h1, hyper


def test_update_skipped_writes_nothing():
    n = 100003
    w, g, m, h = _update_data(n)
    td = lambda z: torch.from_numpy(z.copy()).to(dev())
    for off, cnt in SLICES(n):
        for clip in (0.0, 0.5):
            w1, _, m1, h1, _ = _guarded(w, g, m, h, off, cnt, clip, _state(coef=0.25, skip=1.0))
            assert torch.equal(w1, td(w)) and torch.equal(m1, td(m)) and torch.equal(h1.view(torch.int16), td(h).view(torch.int16)), (off, cnt)


def test_update_inactive_is_the_plain_update_bit_for_bit():
    hip = _hip()
    n = 100003
    w, g, m, h = _update_data(n)
    td = lambda z: torch.from_numpy(z.copy()).to(dev())
    for off, cnt in SLICES(n):
        for clip in (0.0, -1.0):
            w1, g1, m1, h1, hyper = _guarded(w, g, m, h, off, cnt, clip, _state())
            w2, m2, h2 = td(w), td(m), td(h)
            hip.call('sn_sgd_mom_update_dev', w2[off:], g1[off:], m2[off:], h2[off:], cnt, hyper, 2.0, 0.5, hip.stream())
            assert torch.equal(w1, w2) and torch.equal(m1, m2) and torch.equal(h1.view(torch.int16), h2.view(torch.int16)), (off, cnt)
            assert not torch.equal(w1, td(w))


@pytest.mark.parametrize('coef,clip', [(0.25, 0.0), (1.0, 0.5), (0.25, 0.5)])
def test_update_active_matches_the_restatement(coef, clip):
    n = 100003
    w, g, m, h = _update_data(n)
    if clip > 0:
        u = np.float32(0.5) * (np.float32(coef) * g)
        assert (np.abs(u) > clip).any() and (np.abs(u) < clip).any() and ((np.abs(u) == clip).any() or coef != 1.0)
    td = lambda z: torch.from_numpy(z.copy()).to(dev())
    for off, cnt in SLICES(n):
        state = _state(coef=coef)
        w1, _, m1, h1, _ = _guarded(w, g, m, h, off, cnt, clip, state)
        sl = slice(off, off + cnt)
        ww, wm, _ = ref.guarded_update(w[sl], g[sl], m[sl], HYPER, 2.0, 0.5, clip, state.cpu().numpy())
        gw, gm = w1.cpu().numpy(), m1.cpu().numpy()
        assert np.allclose(gw[sl], ww, rtol=RTOL, atol=ATOL) and np.allclose(gm[sl], wm, rtol=RTOL, atol=ATOL), (off, cnt)
        if cnt > 1000:            # (and the guard did something)
            assert not np.allclose(gm[sl], ref.guarded_update(w[sl], g[sl], m[sl], HYPER, 2.0, 0.5, 0.0, _state().cpu().numpy())[1], rtol=1e-3, atol=1e-4)
        assert torch.equal(h1[sl], w1[sl].half())
        for got, orig in ((w1, w), (m1, m), (h1, h)):
            o = td(orig)
            assert torch.equal(got[:off].view(-1), o[:off].view(-1)) and torch.equal(got[off + cnt:], o[off + cnt:]), (off, cnt)


# ------------------------------------------------------------------------------------------------
# step level: the optimizer pass of a small graph, eager and captured
# ------------------------------------------------------------------------------------------------
A_, B_, S_ = 3, 2, 64
F_ = S_ // 8
SHAPES = dict(data=(B_, 3, S_, S_), label=(B_, A_ * F_ * F_), bbox_target=(B_, 4 * A_, F_, F_), bbox_weight=(B_, 4 * A_, F_, F_))
SGD = dict(lr=1e-4, wd=1e-3, momentum=0.9)


@pytest.fixture(scope='module')
def problem():
    """parameters and six batches of the small graph, made once and never changed"""
    import sniper_amd.mx as mx
    from test_gpu_engine import _mini_graph
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
                  bbox_weight=(rs.uniform(size=(B_, 4 * A_, F_, F_)) < 0.2).astype(np.float32)) for _ in range(6)]
    return P, AUX, feeds


def _fixed(sym):
    return [n for n in sym.list_arguments() if any(p in n for p in ('conv0', 'bn0', 'bn_data'))]


def _executor(problem):
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    from sniper_amd.mx import symbol
    from test_gpu_engine import _mini_graph
    symbol._counter().clear()
    sym = _mini_graph(mx, A_)
    ex = Executor(sym, SHAPES, True, _fixed(sym))
    ex.set_params(problem[0], problem[1])
    return ex


def _params(ex):
    out = {'master': ex.arena_master.clone(), 'mom': ex.arena_mom.clone(), 'w16': ex.arena_w16.clone().view(torch.int16)}
    for k, p in ex.params.items():
        if p.trainable and p.wT16 is not None:
            out['wT16.' + k] = p.wT16.clone().view(torch.int16)
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def _gstate(ex):
    return dict(zip(ref.STATE_KEYS, ex.guard['state'].cpu().tolist()))


@pytest.fixture(params=['eager', 'captured'])
def mode(request, monkeypatch):
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', '1' if request.param == 'captured' else '0')
    return request.param


def test_step_guard_without_effect_is_the_plain_step(mode, problem):
    """1: the same gradients through the plain and the guarded optimizer pass (skip_nonfinite only, nothing to skip): masters,
    momentum, fp16 copies and transposed copies bit-equal after every one of four steps (two eager, the capture, a replay)"""
    a, b = _executor(problem), _executor(problem)
    b.set_grad_guard(skip_nonfinite=True)
    assert _same(_params(a), _params(b)) == []
    for i, feed in enumerate(problem[2][:4]):
        a.forward_backward(feed)
        b.arena_grad.copy_(a.arena_grad)
        for ex in (a, b):
            ex.update(lr=SGD['lr'] * (i + 1), wd=SGD['wd'], momentum=SGD['momentum'])
        assert _same(_params(a), _params(b)) == [], i
    assert (a._graph_up is not None) == (b._graph_up is not None) == (mode == 'captured')
    st = _gstate(b)
    assert st['steps'] == 4 and st['skipped'] == 0 and st['coef'] == 1.0 and st['nonfinite'] == 0


def test_step_counts_and_reports_the_norm(mode, problem):
    """2: five guarded steps with a huge clip_global_norm; the last step's sumsq / norm against the restatement on the arena read
    back before the update (the summation orders differ: the bound of the random-data test)"""
    ex = _executor(problem)
    ex.set_grad_guard(clip_global_norm=1e30)
    for i, feed in enumerate(problem[2][:5]):
        ex.forward_backward(feed)
        arena = ex.arena_grad.cpu().numpy()
        ex.update(rescale_grad=0.5, **SGD)
    st = _gstate(ex)
    assert st['steps'] == 5 and st['skipped'] == 0 and st['consecutive'] == 0 and st['coef'] == 1.0
    assert (ex._graph_up is not None) == (mode == 'captured')
    want = ref.guard(arena, 0.5, 1e30, False, np.zeros(8))
    bound = arena.size * 2.0 ** -53
    print('norm device %.17g restated %.17g' % (st['norm'], want[0]))
    assert want[7] > 0 and abs(st['sumsq'] - want[7]) <= bound * want[7] and abs(st['norm'] - want[0]) <= bound * want[0]
    assert st['norm'] == np.sqrt(st['sumsq']) * 0.5


def test_step_with_a_poisoned_gradient_is_skipped(mode, problem):
    """3: inf written into one arena element between forward_backward and update of a step that is (in captured mode) a replay:
    nothing the optimizer pass owns changes; the next clean step moves the parameters and resets the run of skips"""
    ex = _executor(problem)
    ex.set_grad_guard(skip_nonfinite=True)
    for feed in problem[2][:4]:
        ex.forward_backward(feed)
        ex.update(**SGD)
    assert (ex._graph_up is not None) == (ex._graph_fb is not None) == (mode == 'captured')
    before = _params(ex)
    n_up = ex.num_update
    ex.forward_backward(problem[2][4])
    ex.arena_grad[ex.arena_grad.numel() // 2 + 1] = float('inf')
    ex.update(**SGD)
    assert _same(before, _params(ex)) == []
    st = _gstate(ex)
    assert st['skipped'] == 1 and st['skip'] == 1 and st['nonfinite'] == 1 and st['consecutive'] == 1 and st['steps'] == 5
    assert ex.num_update == n_up + 1                       # the schedule counts batches
    ex.forward_backward(problem[2][5])
    ex.update(**SGD)
    moved = _same(before, _params(ex))
    assert 'master' in moved and 'mom' in moved and 'w16' in moved
    st = _gstate(ex)
    assert st['skipped'] == 1 and st['skip'] == 0 and st['consecutive'] == 0 and st['steps'] == 6
    assert torch.isfinite(ex.arena_master).all() and torch.isfinite(ex.arena_mom).all()


def test_step_clipped_to_half_its_norm_is_the_plain_step_on_half_the_gradients(mode, problem):
    """5: clip_global_norm = half the first step's norm: the parameters after the step against the plain update of 0.5 * the same
    gradients (coef = 0.5 up to the 1e-6 of the rule's denominator), at the active-path bound"""
    a, b = _executor(problem), _executor(problem)
    a.forward_backward(problem[2][0])
    b.arena_grad.copy_(a.arena_grad)
    norm = ref.guard(a.arena_grad.cpu().numpy(), 1.0, 0.0, False, np.zeros(8))[0]
    assert np.isfinite(norm) and norm > 1.0
    b.set_grad_guard(clip_global_norm=0.5 * norm)
    a.arena_grad.mul_(0.5)
    a.update(**SGD)
    b.update(**SGD)
    st = _gstate(b)
    assert abs(st['coef'] - 0.5) < 1e-6 and st['coef'] != 1.0
    pa, pb = _params(a), _params(b)
    print('max |momentum| %.3g' % float(pa['mom'].abs().max()))
    assert torch.allclose(pb['master'], pa['master'], rtol=RTOL, atol=ATOL) and torch.allclose(pb['mom'], pa['mom'], rtol=RTOL, atol=ATOL)
    assert torch.equal(b.arena_w16, b.arena_master.half())
    assert not torch.equal(pa['master'], _params(_executor(problem))['master'])


def test_module_gives_up_after_consecutive_skips(problem, caplog):
    """4: max_consecutive_skips = 2, three poisoned steps, synchronised so that every snapshot has landed before the next update:
    the first update inspects nothing, the second sees a run of 1 (and logs the skipped step), the third sees a run of 2 and raises"""
    import sniper_amd.mx as mx
    from test_gpu_engine import _mini_graph
    P, AUX, feeds = problem
    sym = _mini_graph(mx, A_)
    labels = ['label', 'bbox_target', 'bbox_weight']
    mod = mx.mod.Module(sym, data_names=['data'], label_names=labels, context=[mx.gpu(0)], fixed_param_names=_fixed(sym))
    mod.bind(data_shapes=[('data', SHAPES['data'])], label_shapes=[(k, SHAPES[k]) for k in labels], for_training=True)
    mod.init_params(arg_params=P, aux_params=AUX)
    assert mod.grad_guard_state() is None
    mod.init_optimizer(optimizer='sgd', optimizer_params={'learning_rate': 1e-4, 'momentum': 0.9, 'wd': 1e-3, 'skip_nonfinite': True,
                                                          'max_consecutive_skips': 2})
    assert mod.grad_guard_state()['steps'] == 0 and mod.grad_guard_state(wait=False) is None
    before = mod.exe.arena_master.clone()

    def step(feed, poison):
        mod.forward_backward(mx.io.DataBatch(data=[feed['data']], label=[feed[k] for k in labels]))
        if poison:
            mod.exe.arena_grad[11] = float('nan')
        mod.update()
        torch.cuda.synchronize()
    with caplog.at_level(logging.WARNING):
        step(feeds[0], True)
        assert not [r for r in caplog.records if 'gradient guard' in r.getMessage()]
        step(feeds[1], True)
        logged = [r.getMessage() for r in caplog.records if 'gradient guard' in r.getMessage()]
        assert len(logged) == 1 and 'step 1 skipped' in logged[0] and '1 non-finite' in logged[0]
        lag = mod.grad_guard_state(wait=False)
        assert lag['steps'] == 2 and lag['consecutive'] == 2 and lag['skipped_last'] is True
        with pytest.raises(FloatingPointError):
            step(feeds[2], True)
    st = mod.grad_guard_state()
    assert st['steps'] == 3 and st['skipped'] == 3 and st['consecutive'] == 3 and st['nonfinite'] == 1 and st['skipped_last'] is True
    assert sorted(st) == sorted(('norm', 'coef', 'skipped_last', 'nonfinite', 'steps', 'skipped', 'consecutive', 'sumsq'))
    torch.cuda.synchronize()
    assert torch.equal(before, mod.exe.arena_master)
    # a clean step ends the run
    mod.opt['max_consecutive_skips'] = None
    step(feeds[3], False)
    st = mod.grad_guard_state()
    assert st['steps'] == 4 and st['consecutive'] == 0 and not st['skipped_last'] and not torch.equal(before, mod.exe.arena_master)


def test_trainer_with_the_guard_on():
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=2, n_images=4, seed=0, skip_nonfinite=True, clip_global_norm=1e4)
    ex = tr.mod.exe
    assert ex.guard is not None and ex.guard['skip_nonfinite'] == 1 and ex.guard['clip_global_norm'] == 1e4 and ex.guard['clip_gradient'] == 0.0
    before = ex.arena_master.clone()
    for _ in range(3):
        outs = tr.step()
        for o in outs:
            assert np.isfinite(o.asnumpy()).all()
    st = tr.mod.grad_guard_state()
    print('guard state after three R101 steps: %r' % (st,))
    assert st['steps'] == 3 and st['skipped'] == 0 and st['nonfinite'] == 0 and np.isfinite(st['norm']) and st['norm'] > 0
    assert 0 < st['coef'] <= 1.0
    assert torch.isfinite(ex.arena_master).all() and not torch.equal(before, ex.arena_master)
