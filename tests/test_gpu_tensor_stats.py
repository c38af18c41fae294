"""-m gpu: the per-tensor statistics -- sn_tensor_stats against its numpy restatement (tests/tensor_stats_ref.py): one table with every
edge of the peel / body / tail split, of the block trip and of the chunk, bit for bit in fp32 and fp16 at four misalignments; the same
bits for every grid; non-finite elements at every position; the extremes; the early exit behind the guard's skip flag; then the skip
report of a small graph's optimizer pass, eager and captured, and mx.mon.Monitor through Module.fit."""
import ctypes
import logging

import numpy as np
import pytest
import torch

import tensor_stats_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu


def _hip():
    from sniper_amd import hip
    return hip


def _limits():
    out = (ctypes.c_int32 * 6)()
    _hip().lib().call('sn_tensor_stats_limits', out)
    return tuple(int(v) for v in out)          # S (fp32 per trip), C (chunk), max T, 8, S16 (fp16 per trip), grid cap


class Table(object):
    """a segment table planned and uploaded once, with its workspace"""

    def __init__(self, segs):
        L = _hip().lib()
        self.segs = [(int(a), int(b)) for a, b in segs]
        self.T = len(segs)
        seg = np.ascontiguousarray(np.asarray(self.segs, np.int64).reshape(self.T, 2))
        n = ctypes.c_int32(0)
        L.call('sn_tensor_stats_plan', seg.ctypes.data, self.T, None, 0, ctypes.byref(n))
        self.n_items = n.value
        nbytes = L.raw('sn_tensor_stats_plan_bytes')(self.T, self.n_items)
        plan = np.zeros(nbytes // 8 + 1, np.int64)
        L.call('sn_tensor_stats_plan', seg.ctypes.data, self.T, plan.ctypes.data, nbytes, ctypes.byref(n))
        self.plan = torch.from_numpy(plan).to(dev())
        self.ws = torch.zeros(L.raw('sn_tensor_stats_workspace_bytes')(self.T, self.n_items), dtype=torch.uint8, device=dev())

    def run(self, x, max_blocks=0, state=None, only=0, out=None):
        hip = _hip()
        assert x.dtype in (torch.float32, torch.float16) and max(a + b for a, b in self.segs + [(0, 0)]) <= x.numel()
        if out is None:
            out = torch.full((1 + self.T, 8), -7.0, dtype=torch.float64, device=dev())
        hip.call('sn_tensor_stats', x, 1 if x.dtype == torch.float32 else 0, self.plan, self.n_items, self.T, int(max_blocks), state,
                 int(only), self.ws, out, hip.stream())
        return out.cpu().numpy()


def _layout(lens, gap=lambda k: 1 + k % 9):
    segs, off = [], 0
    for k, n in enumerate(lens):
        off += gap(k)
        segs.append((off, n))
        off += n
    return segs, off + 9


def _placed(host, off, dtype):
    """the host array at `off` ELEMENTS behind a 16-byte boundary; NaN in front of it and behind it"""
    buf = torch.full((host.size + off + 16,), float('nan'), dtype=dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + host.size]
    view.copy_(torch.from_numpy(host))
    return view


@pytest.mark.parametrize('dtype,off', [(torch.float32, 0), (torch.float32, 1), (torch.float32, 2), (torch.float32, 3),
                                       (torch.float16, 0), (torch.float16, 1), (torch.float16, 3), (torch.float16, 7)])
def test_every_edge_is_bit_equal_to_the_restatement(dtype, off):
    """tensor lengths around the vector, the block trip (of both element types) and the chunk, laid out with gaps of 1 to 9 elements
    that hold NaN: integer values in [-8, 8], so every fp64 sum is exact in any order and the whole (1 + T, 8) output equals the
    restatement bit for bit; a tensor that read one element of a gap would count a NaN"""
    S, C, _, _, S16, _ = _limits()
    lens = [0, 1, 3, 4, 7, 8, 15, 16, S - 1, S, S + 1, S16 - 1, S16, S16 + 1, C - 1, C, C + 1, 3 * C + 5]
    segs, total = _layout(lens)
    npdt = np.float32 if dtype == torch.float32 else np.float16
    rs = np.random.RandomState(11 + off)
    host = np.full(total, np.nan, npdt)
    for a, n in segs:
        host[a:a + n] = rs.randint(-8, 9, n).astype(npdt)
    tab = Table(segs)
    assert tab.n_items == sum(-(-n // C) for n in lens)
    x = _placed(host, off, dtype)
    got = tab.run(x)
    want = ref.stats(host, segs, C)
    assert want[0].tolist() == [1.0, 0.0, len(lens), 0.0, -1.0, 0.0, 0.0, 0.0] and (want[1:, 5] > 0).sum() >= 10
    assert got.tobytes() == want.tobytes(), (np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])


@pytest.fixture(scope='module')
def normal_case():
    """standard-normal data in a table of short, chunk-sized and many-chunk tensors, made once"""
    _, C, _, _, _, _ = _limits()
    lens = [5, 1000, C + 17, 3 * C + 5, 0, 70000, 8]
    segs, total = _layout(lens)
    host = np.random.RandomState(3).standard_normal(total).astype(np.float32)
    return segs, host, ref.stats(host, segs, C)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_the_grid_does_not_change_a_bit(dtype, normal_case):
    """max_blocks 1, 2, 7 and the default: the four outputs are bit-identical and a second run repeats them.  Against the restatement:
    every term (double)x * x and (double)x is exact, only the additions round, so sumsq is within n * 2^-53 relative and sum within
    n * 2^-53 * sum|x| of ANY other order of adding them; every other field is exact."""
    segs, host, want = normal_case
    _, C, _, _, _, _ = _limits()
    if dtype == torch.float16:
        host = host.astype(np.float16)
        want = ref.stats(host, segs, C)
    tab = Table(segs)
    x = _placed(host, 1, dtype)
    outs = [tab.run(x, mb) for mb in (1, 2, 7, 0, 0)]
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes()
    got = outs[0]
    assert got[0].tolist() == want[0].tolist()
    for (a, n), g, w in zip(segs, got[1:], want[1:]):
        d = host[a:a + n].astype(np.float64)
        print('n %7d sumsq rel %.3g bound %.3g   sum abs %.3g bound %.3g' % (n, abs(g[0] - w[0]) / max(w[0], 1e-300), n * 2.0 ** -53,
                                                                           abs(g[1] - w[1]), n * 2.0 ** -53 * np.abs(d).sum()))
        assert abs(g[0] - w[0]) <= n * 2.0 ** -53 * w[0]
        assert abs(g[1] - w[1]) <= n * 2.0 ** -53 * np.abs(d).sum()
        assert g[2:].tolist() == w[2:].tolist()


def test_non_finite_elements_are_counted_located_and_left_out():
    """inf, -inf and NaN at a tensor's first element, inside the peeled head, in the body, at the last element of a chunk, the first
    of the next, in the tail behind the last 16-byte load and at the last element -- one at a time and three together: count, first
    index and the header exact; the finite fields those of the same data without the poisoned elements"""
    _, C, _, _, _, _ = _limits()
    n = 2 * C + 13                                   # at 1 float behind a boundary: heads of 3; the last chunk: 3 + 2 vectors + a tail of 2
    segs = [(0, 37), (40, n)]
    rs = np.random.RandomState(23)
    clean = rs.randint(-8, 9, 40 + n).astype(np.float32)
    pos = {'first': 0, 'head': 2, 'body': 4099, 'chunk_last': C - 1, 'chunk_first': C, 'next_head': 2 * C + 1, 'tail': n - 2, 'last': n - 1}
    cases = [[(p, v)] for p in pos.values() for v in (np.inf, -np.inf, np.nan)]
    cases.append([(pos['chunk_last'], np.nan), (pos['chunk_first'], np.inf), (pos['last'], -np.inf)])
    cases.append([(pos['tail'], np.inf), (pos['body'], np.nan), (pos['head'], -np.inf)])
    tab = Table(segs)
    for case in cases:
        host = clean.copy()
        for p, v in case:
            host[40 + p] = v
        got = tab.run(_placed(host, 1, torch.float32))
        assert got[0].tolist() == [1.0, 0.0, 2.0, 1.0, 1.0, 0.0, 0.0, 0.0], case
        rest = ref.record(np.delete(clean[40:], [p for p, _ in case]), 1 << 30)
        assert got[2, 2] == len(case) and got[2, 3] == min(p for p, _ in case), (case, got[2])
        assert got[2, [0, 1, 4, 5]].tolist() == rest[[0, 1, 4, 5]].tolist() and got[2, 6] == n, (case, got[2], rest)
        assert got.tobytes() == ref.stats(host, segs, C).tobytes(), case
        assert got[1].tolist() == ref.record(clean[:37], C).tolist()
    host = clean.copy()
    host[3] = np.nan                                  # the first tensor too: the header's first index is the smaller one
    host[40 + pos['body']] = np.inf
    got = tab.run(_placed(host, 1, torch.float32))
    assert got[0].tolist() == [1.0, 0.0, 2.0, 2.0, 0.0, 0.0, 0.0, 0.0] and got[1, 2:4].tolist() == [1.0, 3.0]


def test_extremes():
    """The fp32 subnormals are written as bit patterns and their expected statistics come from integer arithmetic (k * 2^-149 and
    k^2 * 2^-298 are normal doubles): a process in which the oracle has run flushes subnormals on the HOST (torch.set_flush_denormal),
    float32 conversions and comparisons included, so nothing here makes, converts or compares a subnormal float32 on the host."""
    FMAX, ONE, NEG_ONE, HALF, NEG0 = 0x7f7fffff, 0x3f800000, 0xbf800000, 0x3f000000, 0x80000000
    ks = [1, 5, 3, 0x7fffff, 2]                                                  # fp32 subnormals k * 2^-149, the largest among them
    bits = np.array([FMAX, NEG_ONE, HALF] + [0] + ks + [0] + [NEG0, 0, ONE, NEG0, FMAX | NEG0], np.uint32)
    host = bits.view(np.float32)
    segs = [(0, 3), (4, 5), (10, 5)]
    got = Table(segs).run(_placed(host, 0, torch.float32))
    fmax = (2.0 - 2.0 ** -23) * 2.0 ** 127
    # FLT_MAX^2 dwarfs the other terms: every order of adding them rounds to the same double
    assert got[1].tolist() == [fmax * fmax, fmax - 0.5, 0.0, -1.0, fmax, 0.0, 3.0, 0.0]
    # subnormals are neither zero nor flushed: sum k^2 < 2^47 and sum k < 2^24 are exact integers, the powers of two exact scalings
    assert got[2].tolist() == [float(sum(k * k for k in ks)) * 2.0 ** -298, float(sum(ks)) * 2.0 ** -149, 0.0, -1.0,
                               float(max(ks)) * 2.0 ** -149, 0.0, 5.0, 0.0]
    assert got[3].tolist() == [fmax * fmax + 1.0, 1.0 - fmax, 0.0, -1.0, fmax, 3.0, 5.0, 0.0]
    assert got[0].tolist() == [1.0, 0.0, 3.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    h = np.array([65504, 1, -2.0 ** -24, 0, 2.0 ** -24, -2.0 ** -24, 0.0, -0.0, 0, -65504, np.inf], np.float16)
    segs = [(0, 3), (4, 4), (9, 2)]
    got = Table(segs).run(_placed(h, 0, torch.float16))
    want = ref.stats(h, segs, 1 << 20)
    assert got[1, 4] == 65504.0 and got[2, 4] == 2.0 ** -24 and got[2, 5] == 2 and got[2, 0] == 2.0 ** -47
    assert got[3].tolist() == [65504.0 ** 2, -65504.0, 1.0, 1.0, 65504.0, 0.0, 2.0, 0.0]
    assert got.tobytes() == want.tobytes()


def test_only_if_skipped_leaves_everything_untouched_unless_the_guard_skipped(normal_case):
    segs, host, want = normal_case
    tab = Table(segs)
    x = _placed(host, 2, torch.float32)
    plain = tab.run(x)
    sentinel = lambda t: t.view(torch.uint8).fill_(0xA5)
    out = torch.empty((1 + tab.T, 8), dtype=torch.float64, device=dev())
    sentinel(out)
    sentinel(tab.ws)
    state = torch.tensor([1.0, 1.0, 0.0, 0.0, 40.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=dev())
    got = tab.run(x, state=state, only=1, out=out)
    assert (got.view(np.uint8) == 0xA5).all() and bool((tab.ws == 0xA5).all())
    got = tab.run(x, state=state, only=0, out=out)               # a state, not conditional: written, the header carries the counter
    assert got[0].tolist() == [1.0, 40.0, float(tab.T), 0.0, -1.0, 0.0, 0.0, 0.0] and got[1:].tobytes() == plain[1:].tobytes()
    sentinel(out)
    sentinel(tab.ws)
    state[2], state[4] = 1.0, 41.0
    got = tab.run(x, state=state, only=1, out=out)
    assert got[0, 1] == 41.0 and got[1:].tobytes() == plain[1:].tobytes() and got[0, [0, 2, 3, 4]].tolist() == plain[0, [0, 2, 3, 4]].tolist()
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError):
        tab.run(x, state=None, only=1)


# ------------------------------------------------------------------------------------------------
# engine level: the small graph of tests/test_gpu_grad_guard.py (helpers copied)
# ------------------------------------------------------------------------------------------------
A_, B_, S_ = 3, 2, 64
F_ = S_ // 8
SHAPES = dict(data=(B_, 3, S_, S_), label=(B_, A_ * F_ * F_), bbox_target=(B_, 4 * A_, F_, F_), bbox_weight=(B_, 4 * A_, F_, F_))
SGD = dict(lr=1e-4, wd=1e-3, momentum=0.9)
LABELS = ['label', 'bbox_target', 'bbox_weight']


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


def _module(problem, **opt):
    import sniper_amd.mx as mx
    from sniper_amd.mx import symbol
    from test_gpu_engine import _mini_graph
    symbol._counter().clear()
    sym = _mini_graph(mx, A_)
    mod = mx.mod.Module(sym, data_names=['data'], label_names=LABELS, context=[mx.gpu(0)], fixed_param_names=_fixed(sym))
    mod.bind(data_shapes=[('data', SHAPES['data'])], label_shapes=[(k, SHAPES[k]) for k in LABELS], for_training=True)
    mod.init_params(arg_params=problem[0], aux_params=problem[1])
    mod.init_optimizer(optimizer='sgd', optimizer_params=dict({'learning_rate': 1e-4, 'momentum': 0.9, 'wd': 1e-3}, **opt))
    return mod


def _params(ex):
    out = {'master': ex.arena_master.clone(), 'mom': ex.arena_mom.clone(), 'w16': ex.arena_w16.clone().view(torch.int16)}
    for k, p in ex.params.items():
        if p.trainable and p.wT16 is not None:
            out['wT16.' + k] = p.wT16.clone().view(torch.int16)
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def _same_report(got, want):
    """the two dicts field for field; norm = sqrt(sumsq), whose sum the device takes in another order: n * 2^-53 relative (and the root)"""
    if got is None or want is None or got['step'] != want['step'] or len(got['tensors']) != len(want['tensors']):
        return False
    for g, w in zip(got['tensors'], want['tensors']):
        if {k: v for k, v in g.items() if k != 'norm'} != {k: v for k, v in w.items() if k != 'norm'}:
            return False
        if abs(g['norm'] - w['norm']) > (g['numel'] + 4) * 2.0 ** -53 * w['norm']:
            return False
    return True


@pytest.fixture(params=['eager', 'captured'])
def mode(request, monkeypatch):
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', '1' if request.param == 'captured' else '0')
    monkeypatch.delenv('SNIPER_SKIP_REPORT', raising=False)
    monkeypatch.delenv('SNIPER_MONITOR', raising=False)
    return request.param


def test_report_on_with_clean_gradients_is_the_step_with_the_report_off(mode, problem):
    a, b = _executor(problem), _executor(problem)
    a.set_grad_guard(skip_nonfinite=True)
    b.set_grad_guard(skip_nonfinite=True)
    b.set_skip_report(True)
    for i, feed in enumerate(problem[2][:4]):
        a.forward_backward(feed)
        b.arena_grad.copy_(a.arena_grad)
        for ex in (a, b):
            ex.update(lr=SGD['lr'] * (i + 1), wd=SGD['wd'], momentum=SGD['momentum'])
        assert _same(_params(a), _params(b)) == [], i
    assert (a._graph_up is not None) == (b._graph_up is not None) == (mode == 'captured')
    assert not b.skip_report['out'].any()                      # never written: no step was skipped
    assert b.guard['state'].cpu().tolist()[4:6] == [4.0, 0.0]


def test_skip_report_names_the_parameter_of_a_skipped_step(mode, problem, caplog):
    """three clean steps (in captured mode the fourth is a replay), then inf in one element of one parameter's gradient: the step is
    skipped as before and the report lists exactly that parameter; a clean step leaves the report alone; a second poisoned step on
    another parameter replaces it; the lagged warnings name the parameters"""
    import sniper_amd.mx as mx
    _, C, _, _, _, _ = _limits()
    feeds = problem[2]
    mod = _module(problem, skip_nonfinite=True, skip_report=True, max_consecutive_skips=None)
    ex = mod.exe
    assert ex.skip_report is not None and mod.skip_report() is None and mod.skip_report(wait=False) is None
    tab = ex.skip_report['table']
    names = tab['names']
    first, second = 'stage2_unit1_conv2_weight', 'rpn_cls_score_bias'
    assert first in names and second in names

    def step(feed, poison=None):
        mod.forward_backward(mx.io.DataBatch(data=[feed['data']], label=[feed[k] for k in LABELS]))
        arena = None
        if poison is not None:
            name, index, value = poison
            ex.arena_grad[ex.params[name].offset + index] = value
            arena = ex.arena_grad.cpu().numpy()
        mod.update()
        torch.cuda.synchronize()
        return arena
    with caplog.at_level(logging.WARNING):
        for feed in feeds[:3]:
            step(feed)
        assert mod.skip_report() is None
        before = _params(ex)
        arena = step(feeds[3], (first, 5, float('inf')))
        assert (ex._graph_up is not None) == (mode == 'captured')
        assert _same(before, _params(ex)) == []                                   # skipped as before: nothing moved
        rep = mod.skip_report()
        want = ref.report(ref.stats(arena, [tuple(s) for s in tab['segs']], C, step=4), names)
        assert _same_report(rep, want) and rep['step'] == 4 and len(rep['tensors']) == 1, (rep, want)
        t = rep['tensors'][0]
        assert (t['name'], t['nonfinite'], t['first_index'], t['numel']) == (first, 1, 5, ex.params[first].numel)
        assert np.isfinite(t['norm']) and t['norm'] > 0 and t['max_abs'] > 0
        step(feeds[4])                                                            # a clean step: the report stays
        assert _same(before, _params(ex)) != [] and mod.skip_report() == rep
        assert mod.skip_report(wait=False) == rep                                 # (its snapshot landed: the update above polled it)
        arena = step(feeds[5], (second, 0, float('nan')))
        rep2 = mod.skip_report()
        assert _same_report(rep2, ref.report(ref.stats(arena, [tuple(s) for s in tab['segs']], C, step=6), names)), rep2
        assert rep2['step'] == 6 and [(t['name'], t['nonfinite'], t['first_index']) for t in rep2['tensors']] == [(second, 1, 0)]
        step(feeds[0])                                                            # (one more update: it polls the snapshot of step 6)
        assert mod.skip_report(wait=False) == rep2 == mod.skip_report()
    logged = [r.getMessage() for r in caplog.records if 'gradient guard' in r.getMessage()]
    assert [m for m in logged if 'step 4 skipped, 1 non-finite' in m] and [m for m in logged if 'step 6 skipped, 1 non-finite' in m]
    where = [m for m in logged if 'first in' in m]
    assert len(where) == 2, logged
    assert 'step 4' in where[0] and 'first in %s (1 of %d, first at 5)' % (first, ex.params[first].numel) in where[0]
    assert 'step 6' in where[1] and 'first in %s (1 of %d, first at 0)' % (second, ex.params[second].numel) in where[1]
    st = mod.grad_guard_state()
    assert st['steps'] == 7 and st['skipped'] == 2


class _Batches(object):
    """the iterator Module.fit walks: the fixture's batches, once per epoch"""

    def __init__(self, feeds):
        import sniper_amd.mx as mx
        self.provide_data = [('data', SHAPES['data'])]
        self.provide_label = [(k, SHAPES[k]) for k in LABELS]
        self.batches = [mx.io.DataBatch(data=[f['data']], label=[f[k] for k in LABELS]) for f in feeds]

    def __iter__(self):
        return iter(self.batches)

    def reset(self):
        pass


def _fit_with_monitor(problem, monkeypatch, interval, **opt):
    """-> (per batch: the rows toc returned, a download of every monitored tensor taken at the same point, the sn_tensor_stats calls
    the batch issued, the gradient arena of the batch), the module"""
    import sniper_amd.mx as mx
    from sniper_amd import hip
    from sniper_amd.mx import symbol
    from test_gpu_engine import _mini_graph
    pattern = '.*(weight|weight_grad)$'
    calls = []
    real = hip.call

    def counted(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(hip, 'call', counted)
    seen = []

    class Watched(mx.mon.Monitor):
        def tic(self):
            self.n0 = calls.count('sn_tensor_stats')
            super().tic()

        def toc(self):
            armed = self.activated
            rows = super().toc()
            ex = self.exes[0]
            snap = {k: t.detach().cpu().numpy().astype(np.float64).ravel() for k, t in ex.stat_views(pattern)} if armed else {}
            seen.append((rows, snap, calls.count('sn_tensor_stats') - self.n0, ex.arena_grad.cpu().numpy().copy()))
            return rows
    symbol._counter().clear()
    sym = _mini_graph(mx, A_)
    mod = mx.mod.Module(sym, data_names=['data'], label_names=LABELS, context=[mx.gpu(0)], fixed_param_names=_fixed(sym))
    mod.fit(_Batches(problem[2][:4]), eval_metric='acc', optimizer='sgd',
            optimizer_params=dict({'learning_rate': 1e-4, 'momentum': 0.9, 'wd': 1e-3}, **opt), arg_params=problem[0], aux_params=problem[1],
            num_epoch=1, monitor=Watched(interval, pattern=pattern))
    torch.cuda.synchronize()
    return seen, mod


def _check_rows(rows, snap, names, step):
    """every value against the download: the device's sumsq is within n * 2^-53 relative of the fp64 sum (the bound of the kernel test);
    the square root halves a relative error, and the root, the division and the two roots of the comparison value round once each:
    (n / 2 + 4) * 2^-53 relative"""
    assert [r[1] for r in rows] == names and all(r[0] == step for r in rows)
    for _, name, text in rows:
        x = snap[name]
        want = np.sqrt(np.sum(x * x)) / np.sqrt(x.size)
        got = float(text)
        assert want > 0 and abs(got - want) <= (x.size / 2 + 4) * 2.0 ** -53 * want, (name, got, want)


def test_fit_with_a_monitor(mode, problem, monkeypatch):
    seen, mod = _fit_with_monitor(problem, monkeypatch, 2)
    ex = mod.exe
    weights = [n for n in ex.stat_table()['names'] if n.endswith('weight')]
    names = weights + [n + '_grad' for n in weights]
    assert len(weights) >= 8 and weights == [n for n in ex.stat_table('.*(weight|weight_grad)$', '_grad')['names']]
    assert [bool(rows) for rows, _, _, _ in seen] == [True, False, True, False]
    assert [n for _, _, n, _ in seen] == [2, 0, 2, 0]          # one launch pair per arena on an armed batch, nothing otherwise
    for k in (0, 2):
        _check_rows(seen[k][0], seen[k][1], names, k + 1)
    assert mod.exe.num_update == 4


def test_fit_with_a_monitor_while_accumulating(mode, problem, monkeypatch):
    """accumulate = 2, every batch armed: the gradient rows are those of the accumulation arena -- after the second micro-batch the sum
    of two batches, which the gradient arena itself does not hold"""
    seen, mod = _fit_with_monitor(problem, monkeypatch, 1, accumulate=2)
    ex = mod.exe
    assert ex.accum is not None and ex.num_update == 2
    weights = [n for n in ex.stat_table()['names'] if n.endswith('weight')]
    names = weights + [n + '_grad' for n in weights]
    p = ex.params[weights[-1]]
    for k, (rows, snap, n, arena) in enumerate(seen):
        assert n == 2
        _check_rows(rows, snap, names, k + 1)
        own = arena[p.offset:p.offset + p.numel].astype(np.float64)
        if k % 2 == 0:
            assert np.array_equal(snap[p.name + '_grad'], own)                    # first micro-batch of a window: a copy
        else:
            prev = seen[k - 1][3][p.offset:p.offset + p.numel]
            assert not np.array_equal(snap[p.name + '_grad'], own)
            assert np.array_equal(snap[p.name + '_grad'], (prev + arena[p.offset:p.offset + p.numel]).astype(np.float64))
