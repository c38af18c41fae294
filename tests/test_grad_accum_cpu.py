"""CPU: gradient accumulation without a device -- the options Module.init_optimizer, optimizer_params, Trainer and
Executor.set_accumulate take, the C-ABI calls of a window of micro-steps (recorder of tests/golden/make_call_trace.py) against the
committed traces, the Module's window logic over a stub executor, the two entry points in the header and the library, the compiler's
resource remarks, and the restatement (tests/accumulate_ref.py) on hand-written sequences."""
import ctypes
import importlib
import inspect
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import accumulate_ref as ref  # noqa: E402
from make_call_trace import Recorder, _networks, _zeros, load, trace  # noqa: E402

SYMBOLS = ('sn_grad_accumulate_limits', 'sn_grad_accumulate')
BASE = {'learning_rate': 0.1, 'momentum': 0.9, 'wd': 1e-4, 'rescale_grad': 1.0, 'lr_scheduler': None}
BAD = (True, 2.5, 0, -1)
CASE = 'mobilenetv2_e2e/fix_bn=0'
_name = lambda line: line.split('(')[0]


# ------------------------------------------------------------------------------------------------
# options
# ------------------------------------------------------------------------------------------------
def _module():
    import sniper_amd.mx as mx
    return mx.mod.Module(mx.sym.Variable('x'), data_names=['x'], label_names=None)


def test_init_optimizer_parses_accumulate(monkeypatch):
    monkeypatch.delenv('SNIPER_ACCUMULATE', raising=False)
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    assert m.opt['accumulate'] == 1 and m.accumulate_state() == {'k': 1, 'pending': 0, 'updates': 0}
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=4))
    assert m.opt['accumulate'] == 4 and type(m.opt['accumulate']) is int and m.accumulate_state()['k'] == 4
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=np.int64(2)))
    assert m.opt['accumulate'] == 2
    for bad in BAD + ('3', float('nan')):
        with pytest.raises(ValueError):
            _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=bad))


def test_the_environment_variable_counts_only_without_the_key(monkeypatch):
    monkeypatch.setenv('SNIPER_ACCUMULATE', '3')
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    assert m.opt['accumulate'] == 3
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=None))        # (None is absent)
    assert m.opt['accumulate'] == 3
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=1))           # the key wins
    assert m.opt['accumulate'] == 1
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=5))
    assert m.opt['accumulate'] == 5
    for bad in ('0', '-2', '2.5', 'four', 'True'):
        monkeypatch.setenv('SNIPER_ACCUMULATE', bad)
        with pytest.raises(ValueError):
            _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
        _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=2))      # not even read
    monkeypatch.setenv('SNIPER_ACCUMULATE', '')
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    assert m.opt['accumulate'] == 1


def test_optimizer_params_and_trainer_pass_it_on(monkeypatch):
    monkeypatch.delenv('SNIPER_ACCUMULATE', raising=False)
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer, optimizer_params
    cfg = cfgmod.res101_e2e(batch_images=2)
    assert optimizer_params(cfg).get('accumulate') is None          # absent: 1, or what the environment says
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=optimizer_params(cfg))
    assert m.opt['accumulate'] == 1
    cfg.TRAIN.ACCUMULATE = 8
    for dyn, fp16 in ((None, True), (None, False), (True, True)):
        cfg.TRAIN.fp16 = fp16
        if dyn:
            cfg.TRAIN.DYNAMIC_SCALE = True
        assert optimizer_params(cfg)['accumulate'] == 8, (dyn, fp16)
    m.init_optimizer(optimizer='sgd', optimizer_params=optimizer_params(cfg))
    assert m.opt['accumulate'] == 8
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig['accumulate'].default is None
    src = inspect.getsource(Trainer.__init__)
    assert 'cfg.TRAIN.ACCUMULATE = accumulate' in src
    assert 'BATCH_IMAGES' in Trainer.__doc__ and 'rescale_grad = 1 / k' in Trainer.__doc__


def test_set_accumulate_refuses_the_same_values():
    from sniper_amd.engine.executor import Executor
    for bad in BAD + (None, '2', 1.0):
        with pytest.raises(ValueError):
            Executor.set_accumulate(object(), bad)
    assert Executor.check_accumulate(1) == 1 and Executor.check_accumulate(np.int32(7)) == 7


# ------------------------------------------------------------------------------------------------
# lowering
# ------------------------------------------------------------------------------------------------
def _patched(monkeypatch, setup):
    """every Executor built from here on gets setup(ex) right after its construction; -> the list they are appended to"""
    from sniper_amd.engine.executor import Executor
    init = Executor.__init__
    made = []

    def patched(self, *a, **kw):
        init(self, *a, **kw)
        setup(self)
        made.append(self)
    monkeypatch.setattr(Executor, '__init__', patched)
    return made


def _window_trace(mp, k, micro, setup=lambda ex: None):
    """make_call_trace._train_case for CASE with set_accumulate(k) and `micro` micro-steps through forward_backward + accumulate, then
    one update: phases setup, refresh, (forward, backward, accumulate) x micro, update.  -> (phases, executor, recorder)"""
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.mx import symbol as symmod
    from sniper_amd.train import fixed_param_names
    for key in [key for key in os.environ if key.startswith('SNIPER_')]:
        mp.delenv(key)
    symmod._counter().clear()
    rec = Recorder(mp)
    name = CASE.split('/')[0]
    preset, shapes = _networks()[name]
    cfg = getattr(cfgmod, preset)(batch_images=2)
    cls = getattr(importlib.import_module('sniper_amd.symbols.faster.' + name), name)
    sym = cls(momentum=0.995, fix_bn=False).get_symbol_rcnn(cfg)
    rec.phase('setup')
    ex = Executor(sym, shapes, True, fixed_param_names(cfg, sym), device=torch.device('cpu'))
    setup(ex)
    ex.set_accumulate(k)
    ex.use_graphs = False
    rec.name_tensors(ex)
    rec.own(ex.accum['arena'], 'accum')
    rec.phase('refresh')
    ex.refresh_compute_copies()
    rec.phase('inputs')
    ex.load_inputs(_zeros(shapes))
    rec.name_tensors(ex)
    assert rec.phases.pop() == ['inputs', []]              # (a host copy: no C-ABI call)
    backward = ex.backward

    def backward_phase(*a, **kw):
        rec.phase('backward')
        return backward(*a, **kw)
    ex.backward = backward_phase
    for i in range(micro):
        rec.phase('forward')
        ex.forward_backward(_zeros(shapes))
        rec.phase('accumulate')
        assert ex.accumulate() == i + 1
    rec.phase('update')
    ex.update(0.01, 1e-4, 0.9, 1.0)
    return rec.phases, ex, rec


def _on_the_accumulation_arena(line, ex, rec):
    """a committed guard / SGD line with its gradient operand moved from the gradient arena to the accumulation arena"""
    n = ex.arena_grad.numel()
    for (_lr, _wd, _half), a, b in [((0, 0, 0), 0, n)] + list(ex.groups):
        old, new = rec.arg(ex.arena_grad[a:]), rec.arg(ex.accum['arena'][a:])
        assert old.startswith('par.') and new.startswith('accum')
        if old in line:
            return line.replace(old, new)
    return line


def test_off_again_is_the_committed_trace(monkeypatch):
    """set_accumulate(3); set_accumulate(1): nothing is left of it -- the committed trace, every phase"""
    def on_then_off(ex):
        ex.set_accumulate(3)
        assert ex.accum['k'] == 3 and ex.accum['pending'] == 0 and ex.accum['arena'].shape == ex.arena_grad.shape
        assert ex.accum['arena'].dtype == torch.float32 and ex.grad_arena() is ex.accum['arena']
        ex.set_accumulate(1)
        assert ex.accum is None and ex.grad_arena() is ex.arena_grad
    made = _patched(monkeypatch, on_then_off)
    assert trace(CASE, monkeypatch) == load()[CASE]
    assert len(made) == 1
    with pytest.raises(RuntimeError):
        made[0].accumulate()


def _check_window(got, want, ex, rec, k=2, micro=2, shadow_first=None):
    """got: _window_trace's phases; want: the phases of the same executor settings without accumulation (a committed trace, or the
    guard's / the scaler's)"""
    by = dict((p, lines) for p, lines in want)
    assert [p for p, _ in got] == ['setup', 'refresh'] + ['forward', 'backward', 'accumulate'] * micro + ['update']
    assert got[0][1] == by['setup'] and got[1][1] == by['refresh']
    n = ex.arena_grad.numel()
    assert n == max(ex.n_trainable, 8)
    for i in range(micro):
        fwd, bwd, acc = (got[2 + 3 * i + j][1] for j in range(3))
        if shadow_first is not None:
            # the save of the moving statistics: in the committed-style trace the first line of every forward; here an eager launch
            # before the first micro-step of the window, and nowhere else
            assert by['forward'][0] == shadow_first
            assert fwd == (by['forward'] if i == 0 else by['forward'][1:]), i
        else:
            assert fwd == by['forward'], i
        want_bwd = by['backward']
        if i > 0:
            # the recorder writes the CURRENT size of the executor's grow-only scratch buffer (hip.Workspace): in a later micro-step it
            # is what the largest earlier launch left it at, in a first step what each launch grew it to -- the one thing that may
            # differ; the launches, their order and every other argument may not
            bwd, want_bwd = ([re.sub(r'tmp:uint8:\(\d+,\)', 'tmp:uint8:(ws)', l) for l in lines] for lines in (bwd, want_bwd))
        assert bwd == want_bwd, i
        grad0 = rec.arg(ex.arena_grad)
        assert acc == ['sn_grad_accumulate(accum:float32:(%d,), %s, %d, %d, 0, None)' % (n, grad0, n, 1 if i == 0 else 0)], i
        assert grad0.startswith('par.') and grad0.endswith('.grad:float32:(%d,)' % n)
    up, up0 = got[-1][1], by['update']
    assert len(up) == len(up0)
    moved = 0
    for a, b in zip(up, up0):
        if _name(b) in ('sn_grad_guard', 'sn_grad_guard_scaled', 'sn_sgd_mom_update_dev', 'sn_sgd_mom_update_guarded_dev'):
            want_line = _on_the_accumulation_arena(b, ex, rec)
            assert want_line != b and a == want_line, (a, b)
            moved += 1
        else:
            assert a == b
    guards = sum(1 for l in up0 if _name(l) in ('sn_grad_guard', 'sn_grad_guard_scaled'))
    assert moved == len(ex.groups) + guards and len(ex.groups) >= 2
    assert not [l for l in up if 'accum' not in l and '.grad' in l and _name(l) != 'sn_ew_f32']
    assert ex.accum['pending'] == 0 and ex.num_update == 1 and ex._graph_fb is None


def test_window_of_two_lowering(monkeypatch):
    got, ex, rec = _window_trace(monkeypatch, 2, 2)
    _check_window(got, load()[CASE], ex, rec)
    with pytest.raises(RuntimeError):
        ex.update(0.01, 1e-4, 0.9, 1.0)                    # nothing pending


def test_partial_window_lowering(monkeypatch):
    """k = 3, one micro-step, update: whatever is pending is applied"""
    got, ex, rec = _window_trace(monkeypatch, 3, 1)
    _check_window(got, load()[CASE], ex, rec, k=3, micro=1)


def test_window_lowering_with_the_guard(monkeypatch):
    setup = lambda ex: ex.set_grad_guard(clip_gradient=0.5, clip_global_norm=35.0, skip_nonfinite=True)
    with pytest.MonkeyPatch.context() as mp:
        _patched(mp, setup)
        theirs = trace(CASE, mp)
    got, ex, rec = _window_trace(monkeypatch, 2, 2, setup)
    assert [_name(l) for l in theirs[-1][1]].count('sn_grad_guard') == 1
    _check_window(got, theirs, ex, rec)


@pytest.mark.parametrize('restore_aux', [True, False])
def test_window_lowering_with_dynamic_loss_scale(monkeypatch, restore_aux):
    setup = lambda ex: ex.set_loss_scale(128.0, growth_interval=7, max_scale=2.0 ** 20, restore_aux=restore_aux)
    with pytest.MonkeyPatch.context() as mp:
        _patched(mp, setup)
        theirs = trace(CASE, mp)
    got, ex, rec = _window_trace(monkeypatch, 2, 2, setup)
    ls = ex.loss_scale
    shadow = None
    if restore_aux:
        assert ls['n_aux'] > 0
        shadow = 'sn_aux_shadow(tmp:uint8:(%d,), %d, tmp:float32:(%d,), 0, None, None)' % (16 * ls['n_aux'], ls['n_aux'], ls['shadow'].numel())
    else:
        assert ls['n_aux'] == 0
    _check_window(got, theirs, ex, rec, shadow_first=shadow)
    saves = [l for _, lines in got for l in lines if _name(l) == 'sn_aux_shadow' and ', 0, None, None)' in l]
    assert len(saves) == (1 if restore_aux else 0)         # once per window
    assert [_name(l) for l in got[-1][1]].count('sn_grad_guard_scaled') == 1


def test_set_accumulate_drops_the_graphs_it_must(monkeypatch):
    """both directions drop the optimizer graph (it holds the arena's address); the forward/backward graph goes only where the save of
    the moving statistics moves out of, or back into, the forward body"""
    from sniper_amd import hip
    monkeypatch.setattr(hip, 'call', lambda *a: 0)
    monkeypatch.setattr(hip, 'stream', lambda: None)
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    from sniper_amd.mx import symbol as symmod
    symmod._counter().clear()
    x = mx.sym.FullyConnected(data=mx.sym.Variable('data'), num_hidden=8, name='fc')
    sym = mx.sym.SoftmaxOutput(data=x, label=mx.sym.Variable('label'), name='prob', grad_scale=1.0)
    ex = Executor(sym, dict(data=(4, 16), label=(4,)), True, [], device=torch.device('cpu'))
    for k in (2, 3, 1, 1):
        ex._graph_fb, ex._graph_up = 'fb', 'up'
        ex.set_accumulate(k)
        assert ex._graph_fb == 'fb' and ex._graph_up is None, k
        assert (ex.accum is None) == (k == 1)
    ex.set_loss_scale(128.0)
    ex.loss_scale['n_aux'] = 2                             # (as with batch-statistics BatchNorms in the graph)
    for k, fb in ((2, None), (3, 'fb'), (1, None), (1, 'fb')):
        ex._graph_fb, ex._graph_up = 'fb', 'up'
        ex.set_accumulate(k)
        assert ex._graph_fb == fb and ex._graph_up is None, k


# ------------------------------------------------------------------------------------------------
# Module window logic over a stub executor
# ------------------------------------------------------------------------------------------------
class _StubExe(object):
    for_training = True
    split_k = 5
    guard = loss_scale = None
    input_names = ['x']
    ar_ranges = [(0, False, 0, 40), (1, False, 40, 64)]

    def __init__(self):
        self.arena_grad, self.arena = torch.zeros(64), torch.zeros(64)
        self.arena_mom = torch.zeros(64)
        self.accum, self.num_update, self.log, self.pending = None, 0, [], 0

    def set_accumulate(self, k):
        self.accum = None if k == 1 else {'k': k}
        self.log.append(('set_accumulate', k))

    def forward_backward(self, feed, between=None):
        self.log.append(('forward_backward', between))

    def accumulate(self):
        self.pending += 1
        self.log.append(('accumulate', self.pending))
        return self.pending

    def update(self, lr, wd, momentum, rescale_grad):
        self.num_update += 1
        self.pending = 0
        self.log.append(('update', lr))

    def grad_arena(self):
        return self.arena if self.accum is not None else self.arena_grad

    def get_params(self):
        return {}, {}


class _Dist(object):
    @staticmethod
    def get_world_size():
        return 2


def test_module_window_logic(monkeypatch, tmp_path, caplog):
    import sniper_amd.mx as mx
    from sniper_amd import parallel
    modmod = sys.modules[mx.mod.Module.__module__]
    reduced, sched_calls = [], []
    monkeypatch.delenv('SNIPER_ACCUMULATE', raising=False)
    monkeypatch.setattr(modmod, '_dist', lambda: _Dist)
    monkeypatch.setattr(parallel, 'allreduce_ranges', lambda arena, ranges, d, half_buf=None: reduced.append((arena, list(ranges))))

    def sched(num_update):
        sched_calls.append(num_update)
        return 0.01 * num_update
    m = _module()
    ex = _StubExe()
    m.exe, m._exes, m._device, m.for_training, m.binded = ex, {'only': ex}, torch.device('cpu'), True, True
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, accumulate=3, lr_scheduler=sched))
    assert ex.log == [('set_accumulate', 3)]
    batch = mx.io.DataBatch(data=[np.zeros((2, 4), np.float32)], label=None)
    at = []
    for call in range(1, 8):
        m.forward_backward(batch)
        assert ex.log[-1] == ('forward_backward', None)                   # no overlap while accumulating, split or not
        n_red, n_sched, n_up = len(reduced), len(sched_calls), ex.num_update
        m.update()
        did = (len(reduced) - n_red, len(sched_calls) - n_sched, ex.num_update - n_up)
        assert did in ((0, 0, 0), (1, 1, 1)), (call, did)
        if did[0]:
            at.append(call)
    assert at == [3, 6] and sched_calls == [1, 2]
    for arena, ranges in reduced:
        assert arena is ex.arena and ranges == [(False, 0, 40), (False, 40, 64)]      # the accumulation arena, every range, once
    assert [e for e in ex.log if e[0] == 'accumulate'] == [('accumulate', p) for p in (1, 2, 3, 1, 2, 3, 1)]
    assert [e for e in ex.log if e[0] == 'update'] == [('update', 0.01), ('update', 0.02)]
    assert m.accumulate_state() == {'k': 3, 'pending': 1, 'updates': 2}
    with caplog.at_level(logging.WARNING):
        m.save_checkpoint(str(tmp_path / 'ck'), 1, save_optimizer_states=False)
        assert not [r for r in caplog.records if 'accumulation' in r.getMessage()]
        m.save_checkpoint(str(tmp_path / 'ck'), 1, save_optimizer_states=True)
    warned = [r.getMessage() for r in caplog.records if 'accumulation' in r.getMessage()]
    assert len(warned) == 1 and '1 of 3' in warned[0] and 'new window' in warned[0]
    # k = 1 again: today's update, every call
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, lr_scheduler=sched))
    assert ex.log[-1] == ('set_accumulate', 1) and m.accumulate_state() == {'k': 1, 'pending': 0, 'updates': 0}
    m.forward_backward(batch)
    assert ex.log[-1][0] == 'forward_backward' and ex.log[-1][1] is not None       # the overlap is back
    m._comm_event = None
    m.update()
    assert ex.log[-1][0] == 'update' and len(reduced) == 3 and reduced[-1][0] is ex.arena_grad
    assert m.accumulate_state() == {'k': 1, 'pending': 0, 'updates': 1}


# ------------------------------------------------------------------------------------------------
# build checks
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_accumulation():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import SniperHipError, lib
    L = lib()
    hdr = open(os.path.join(ROOT, 'include', 'sniper_hip.h')).read()
    dll = ctypes.CDLL(os.path.join(ROOT, 'sniper_amd', 'lib', 'libsniper_hip.so'))
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, hdr) and s in L.protos and hasattr(dll, s), s
    assert len(L.protos['sn_grad_accumulate'][1]) == 6 and len(L.protos['sn_grad_accumulate_limits'][1]) == 1
    lim = (ctypes.c_int32 * 3)()
    L.call('sn_grad_accumulate_limits', lim)
    T, F, cap = (int(v) for v in lim)
    assert T % 64 == 0 and F % 4 == 0 and 256 <= cap <= 65535
    with pytest.raises(SniperHipError):
        L.call('sn_grad_accumulate_limits', None)
    # argument errors are reported before any launch (there is no device here: a launch would fail with another message)
    a, g = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21)
    for args in ((None, g, 4, 1, 0, None), (a, None, 4, 0, 0, None), (a, g, -1, 1, 0, None), (ctypes.c_void_p((1 << 20) + 2), g, 4, 1, 0, None),
                 (a, ctypes.c_void_p((1 << 21) + 1), 4, 0, 0, None), (a, g, 4, 1, -1, None), (a, g, 4, 1, 65536, None),
                 (a, a, 4, 0, 0, None), (a, ctypes.c_void_p((1 << 20) + 12), 4, 1, 0, None), (ctypes.c_void_p((1 << 20) + 4), a, 2, 1, 0, None)):
        with pytest.raises(SniperHipError) as e:
            L.call('sn_grad_accumulate', *args)
        assert 'sn_grad_accumulate' in str(e.value) and 'failed (1)' in str(e.value), args          # SN_ERR_ARG
    assert L.call('sn_grad_accumulate', a, g, 0, 1, 0, None) == 0 and L.call('sn_grad_accumulate', None, None, 0, 0, 0, None) == 0


def test_accumulate_kernels_keep_registers_and_occupancy():
    """the compiler's resource remarks the build keeps beside the object: every form of the stream kernel (copy / add, 16-byte or
    4-byte gradient loads) runs eight waves per SIMD with nothing in scratch memory, and uses no LDS"""
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from test_kernel_resources import _resources
    res = _resources('grad_accum')
    hits = {k: v for k, v in res.items() if 'grad_accum_kernel' in k}
    assert len(hits) == len(res) == 4, sorted(res)
    for name, r in hits.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0 and r['Occupancy'] == 8, (name, r)
        lds = [v for k, v in r.items() if 'LDS' in k]
        assert lds and not any(lds), (name, r)


# ------------------------------------------------------------------------------------------------
# the restatement on hand-written sequences
# ------------------------------------------------------------------------------------------------
def test_restated_accumulate():
    """by bit patterns: the restatement must hold in a process whose host arithmetic flushes subnormals (the oracle turns
    torch.set_flush_denormal on), so nothing here makes or compares a subnormal as a float"""
    f = lambda *patterns: ref.from_bits(list(patterns))
    g = f(0x3fc00000, 0x80000000, 0x7f800000, 0x7fc12345, 0x00000001, 0x7f7fffff, 0x00800000, 0x3f800000, 0x3f800000, 0x00200000)
    first = ref.accumulate(np.full(g.size, 9.0, np.float32), g, True)
    assert first.tobytes() == g.tobytes() and first is not g                 # NaN payload, -0 and the subnormal included
    assert ref.accumulate(None, f(0xffc00001), True).tobytes() == f(0xffc00001).tobytes()
    h = f(0x3e800000, 0x00000000, 0xff800000, 0x3f800000, 0x00000001, 0x7f7fffff, 0x80000001, 0x33800000, 0x33c00000, 0x00300000)
    s = ref.bits(ref.accumulate(first, h, False))
    assert s[0] == 0x3fe00000 and s[1] == 0                                   # 1.5 + 0.25; -0 + +0 = +0
    assert s[2] & 0x7f800000 == 0x7f800000 and s[2] & 0x7fffff and s[3] & 0x7f800000 == 0x7f800000 and s[3] & 0x7fffff      # NaN, NaN
    assert s[4] == 2 and s[5] == 0x7f800000                                   # subnormals kept; FLT_MAX + FLT_MAX = inf
    assert s[6] == 0x007fffff and s[9] == 0x00500000                          # 2^-126 - tiny and 2^-128 + 1.5 * 2^-128: subnormal sums
    assert s[7] == 0x3f800000 and s[8] == 0x3f800001                          # 1 + 2^-24: the tie goes to even; 1 + 1.5 * 2^-24: up
    assert ref.accumulate(f(0x80000000), f(0x80000000), False).tobytes() == f(0x80000000).tobytes()
    # against numpy's own float32 addition where no subnormal is involved (any host mode adds those alike)
    rs = np.random.RandomState(1)
    a, b = (ref.from_bits((rs.randint(0, 2, 100000).astype(np.uint32) << 31) | (rs.randint(90, 165, 100000).astype(np.uint32) << 23) |
                          rs.randint(0, 1 << 23, 100000).astype(np.uint32)) for _ in range(2))
    assert ref.same_bits(ref.accumulate(a, b, False), a + b)
    res = ref.from_bits(s)
    assert ref.same_bits(res, res.copy()) and not ref.same_bits(res, ref.from_bits(np.where(s == 2, 0, s)))
    assert not ref.same_bits(f(0), f(0x80000000)) and ref.same_bits(f(0x7fc00000), f(0xffc12345))


def test_restated_windows_a_poisoned_one_is_skipped_and_the_scale_halves_once():
    """hand-written: k = 3, scale 2^10, lr 0.5, no momentum, no decay; gradients arrive times the scale.  Window 1 holds an inf in its
    second micro-batch: skipped as a whole, the scale halves ONCE, the moving statistics go back to what they were before the window's
    first micro-batch.  Window 2 (at 2^9) updates with the true sum."""
    aux = [np.array([1.0, 2.0], np.float32)]
    win = ref.Window(3, (0.5, 0.0, 0.0, 1.0), loss_scale=dict(init_scale=1024.0, growth_interval=0), aux=aux)
    w, mom = np.array([1.0, -1.0, 0.5, 0.0], np.float32), np.zeros(4, np.float32)
    true = [np.array(v, np.float32) for v in ([1, 0, 0, 2], [0, 1, 0, 2], [0, 0, 1, 2])]
    for i, t in enumerate(true):
        win.before_forward()
        aux[0] += 1.0                                       # the forward rewrites the moving statistics
        assert win.scale() == 1024.0                        # one scale for the whole window
        g = t * np.float32(win.scale())
        if i == 1:
            g[2] = np.inf
        assert win.micro(g) == i + 1
    assert aux[0].tolist() == [4.0, 5.0]
    nw, nm, _ = win.update(w, mom)
    assert np.array_equal(nw, w) and np.array_equal(nm, mom) and win.pending == 0
    st = dict(zip(ref.gref.STATE_KEYS, win.state))
    assert (st['steps'], st['skipped'], st['consecutive'], st['nonfinite'], st['skip']) == (1, 1, 1, 1, 1)
    ls = dict(zip(ref.lref.LS_KEYS, win.ls))
    assert (ls['scale'], ls['scale_used'], ls['backoffs'], ls['clean']) == (512.0, 1024.0, 1, 0)
    assert aux[0].tolist() == [1.0, 2.0]                    # as before the window, not as before its last micro-batch
    with pytest.raises(RuntimeError):
        win.update(w, mom)
    for t in true:
        win.before_forward()
        aux[0] += 1.0
        assert win.scale() == 512.0
        win.micro(t * np.float32(win.scale()))
    assert win.acc.tolist() == [512.0, 512.0, 512.0, 3072.0]
    nw, nm, h = win.update(w, mom)
    assert nm.tolist() == [-0.5, -0.5, -0.5, -3.0] and nw.tolist() == [0.5, -1.5, 0.0, -3.0] and np.array_equal(h, nw.astype(np.float16))
    st = dict(zip(ref.gref.STATE_KEYS, win.state))
    assert (st['steps'], st['skipped'], st['consecutive'], st['skip']) == (2, 1, 0, 0) and st['norm'] == np.sqrt(39.0)
    ls = dict(zip(ref.lref.LS_KEYS, win.ls))
    assert (ls['scale'], ls['scale_used'], ls['backoffs'], ls['clean']) == (512.0, 512.0, 1, 1)
    assert aux[0].tolist() == [4.0, 5.0] and win.updates == 2


def test_restated_window_sums_in_arrival_order_and_flushes_a_partial_window():
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    win = ref.Window(3, (1.0, 0.0, 0.0, 1.0))
    for g in (big, one, one):
        win.micro(np.array([g], np.float32))
    assert win.acc[0] == big                                # (2^24 + 1) + 1 in float32, not 2^24 + (1 + 1)
    w, m, _ = win.update(np.zeros(1, np.float32), np.zeros(1, np.float32))
    assert w[0] == -big and not win.guarded and win.state.tolist() == [0.0] * 8
    win.micro(np.array([3.0], np.float32))
    win.micro(np.array([4.0], np.float32))
    w, m, _ = win.update(np.zeros(1, np.float32), np.zeros(1, np.float32))       # two of three pending: the update on g1 + g2
    assert w[0] == -7.0 and win.updates == 2
    clip = ref.Window(2, (1.0, 0.0, 0.0, 1.0), clip_global_norm=2.5)
    clip.micro(np.array([3.0, 0.0], np.float32))
    clip.micro(np.array([0.0, 4.0], np.float32))
    w, _, _ = clip.update(np.zeros(2, np.float32), np.zeros(2, np.float32))      # the clip acts on the sum: norm 5 -> coef 0.5
    assert np.allclose(w, [-1.5, -2.0], rtol=1e-6) and abs(clip.state[1] - 0.5) < 1e-6
