"""CPU: the gradient guard without a device -- its numpy restatement against torch.nn.utils.clip_grad_norm_, the optimizer
parameters Module.init_optimizer parses, the C-ABI calls a guarded optimizer pass issues (recorder of tests/golden/make_call_trace.py),
and the four entry points in the header and the library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import grad_guard_ref as ref  # noqa: E402
from make_call_trace import load, trace  # noqa: E402

SYMBOLS = ('sn_grad_guard_limits', 'sn_grad_guard_workspace_bytes', 'sn_grad_guard', 'sn_sgd_mom_update_guarded_dev')


@pytest.mark.parametrize('where', ['below', 'on', 'above'])
def test_coef_is_the_rule_of_clip_grad_norm(where):
    """the clipped gradients coef * g of the restatement against torch.nn.utils.clip_grad_norm_ on CPU tensors, at the bound the
    device tests use for one-ulp differences (torch scales in float32 by a float32 coefficient)"""
    rs = np.random.RandomState(3)
    parts = [rs.standard_normal(s).astype(np.float32) for s in ((7, 5), (33,), (2, 3, 4))]
    flat = np.concatenate([p.ravel() for p in parts])
    norm = float(np.sqrt(np.sum(flat.astype(np.float64) ** 2)))
    clip = {'below': 2.0 * norm, 'on': float(np.float32(norm)), 'above': 0.25 * norm}[where]
    st = ref.guard(flat, 1.0, clip, False, np.zeros(8))
    assert st[0] == np.sqrt(st[7]) and st[3] == 0 and st[2] == 0 and st[4] == 1
    if where == 'below':
        assert st[1] == 1.0
    if where == 'above':
        assert abs(st[1] - 0.25) < 1e-6
    ps = [torch.nn.Parameter(torch.zeros(p.shape)) for p in parts]
    for p, g in zip(ps, parts):
        p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_(ps, clip)
    assert abs(float(total) - st[0]) <= 1e-6 * st[0]
    got = np.concatenate([p.grad.numpy().ravel() for p in ps])
    assert np.allclose(np.float32(st[1]) * flat, got, rtol=1e-6, atol=1e-7)


def test_restatement_counts_and_counters():
    g = np.array([3.0, np.inf, -4.0, np.nan, -np.inf, 0.0], np.float32)
    st = ref.guard(g, -2.0, 5.0, True, np.zeros(8))
    assert st.tolist() == [10.0, 5.0 / (10.0 + 1e-6), 1.0, 3.0, 1.0, 1.0, 1.0, 25.0]
    st = ref.guard(g, -2.0, 5.0, True, st)
    assert st[4:7].tolist() == [2.0, 2.0, 2.0]
    st = ref.guard(g[[0, 2, 5]], -2.0, 0.0, True, st)
    assert st.tolist() == [10.0, 1.0, 0.0, 0.0, 3.0, 2.0, 0.0, 25.0]
    assert ref.guard(g, 1.0, None, False, np.zeros(8))[2] == 0.0           # counted, not skipped
    w, m = np.ones(6, np.float32), np.zeros(6, np.float32)
    nw, nm, h = ref.guarded_update(w, g, m, (0.1, 0.0, 0.9, 1.0), 1.0, 1.0, None, [0, 1, 1, 0, 0, 0, 0, 0])
    assert np.array_equal(nw, w) and np.array_equal(nm, m)                 # skip: nothing moves
    nw, nm, h = ref.guarded_update(w, np.array([4, -4, 0.5, 1, -1, 0], np.float32), m, (0.5, 0.0, 0.0, 2.0), 1.0, 1.0, 1.0,
                                   [0, 0.5, 0, 0, 0, 0, 0, 0])
    assert nm.tolist() == [-0.5, 0.5, -0.25, -0.5, 0.5, 0.0] and np.array_equal(h, nw.astype(np.float16))


def _module():
    import sniper_amd.mx as mx
    return mx.mod.Module(mx.sym.Variable('x'), data_names=['x'], label_names=None)


def test_init_optimizer_parses_the_guard_options():
    base = {'learning_rate': 0.1, 'momentum': 0.9, 'wd': 1e-4, 'rescale_grad': 1.0, 'lr_scheduler': None}
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(base))
    assert m.opt['guard'] is False and m.opt['max_consecutive_skips'] == 16 and m.grad_guard_state() is None
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(base, clip_gradient=None, clip_global_norm=None, skip_nonfinite=False))
    assert m.opt['guard'] is False                       # what the reference passes: clip_gradient None
    for key, val in (('clip_gradient', 0.5), ('clip_global_norm', 10), ('skip_nonfinite', True)):
        m = _module()
        m.init_optimizer(optimizer='sgd', optimizer_params=dict(base, **{key: val}))
        assert m.opt['guard'] is True and m.opt[key] == val
        assert [m.opt[k] for k in ('clip_gradient', 'clip_global_norm', 'skip_nonfinite') if k != key] in ([None, None], [None, False])
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(base, skip_nonfinite=True, max_consecutive_skips=None))
    assert m.opt['max_consecutive_skips'] is None
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(base, skip_nonfinite=True, max_consecutive_skips=3))
    assert m.opt['max_consecutive_skips'] == 3
    for key in ('clip_gradient', 'clip_global_norm'):
        for bad in (0, 0.0, -1.0, float('nan'), 'big', True):
            with pytest.raises(ValueError):
                _module().init_optimizer(optimizer='sgd', optimizer_params=dict(base, **{key: bad}))
    for key, bad in (('skip_nonfinite', 'yes'), ('skip_nonfinite', 2), ('max_consecutive_skips', 0), ('max_consecutive_skips', 1.5)):
        with pytest.raises(ValueError):
            _module().init_optimizer(optimizer='sgd', optimizer_params=dict(base, **{key: bad}))


def test_optimizer_params_and_trainer_pass_the_options_on():
    import inspect
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer, optimizer_params
    cfg = cfgmod.res101_e2e(batch_images=2)
    op = optimizer_params(cfg)
    assert op['clip_gradient'] is None and op['clip_global_norm'] is None and op['skip_nonfinite'] is False
    cfg.TRAIN.CLIP_GRADIENT, cfg.TRAIN.CLIP_GLOBAL_NORM, cfg.TRAIN.SKIP_NONFINITE = 2.0, 35.0, True
    op = optimizer_params(cfg)
    assert (op['clip_gradient'], op['clip_global_norm'], op['skip_nonfinite']) == (2.0, 35.0, True)
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=op)
    assert m.opt['guard'] is True
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig['clip_gradient'].default is None and sig['clip_global_norm'].default is None and sig['skip_nonfinite'].default is False


CASE = 'mobilenetv2_e2e/fix_bn=0'


def test_guarded_update_lowering(monkeypatch):
    """A guarded eager optimizer pass: one sn_grad_guard over the whole gradient arena, then one sn_sgd_mom_update_guarded_dev per
    group on the buffers and multipliers of the unguarded trace's sn_sgd_mom_update_dev lines, no sn_sgd_mom_update_dev; everything
    before and after the updates is the unguarded trace."""
    from sniper_amd.engine.executor import Executor
    plain = load()[CASE]
    init = Executor.__init__
    made = []

    def guarded_init(self, *a, **kw):
        init(self, *a, **kw)
        self.set_grad_guard(clip_gradient=0.5, clip_global_norm=35.0, skip_nonfinite=True)
        made.append(self)
    monkeypatch.setattr(Executor, '__init__', guarded_init)
    got = trace(CASE, monkeypatch)
    assert [p for p, _ in got] == [p for p, _ in plain] and got[-1][0] == 'update'
    for (phase, a), (_, b) in zip(got[:-1], plain[:-1]):
        assert a == b, phase
    ex = made[0]
    n = ex.arena_grad.numel()
    assert ex.guard is not None and n == max(ex.n_trainable, 8)
    assert tuple(ex.guard['state'].shape) == (8,) and ex.guard['state'].dtype == torch.float64 and not ex.guard['state'].any()
    from sniper_amd import hip
    assert ex.guard['ws'].numel() >= hip.query('sn_grad_guard_workspace_bytes', n, 0) > 0
    up, want = got[-1][1], plain[-1][1]
    name = lambda line: line.split('(')[0]
    first = [name(l) for l in want].index('sn_sgd_mom_update_dev')
    assert up[:first] == want[:first]                                    # the hyper-parameter fills
    groups = [l for l in want if name(l) == 'sn_sgd_mom_update_dev']
    assert len(groups) == len(ex.groups) >= 2
    assert name(up[first]) == 'sn_grad_guard'
    args = up[first][len('sn_grad_guard('):-1]
    assert args.startswith('par.') and ':float32:(%d,), %d, tmp:float32:(4,), 35.0, 1, 0, tmp:uint8:' % (n, n) in args
    assert args.endswith('tmp:float64:(8,), None')
    assert [name(l) for l in up].count('sn_grad_guard') == 1 and not [l for l in up if name(l) == 'sn_sgd_mom_update_dev']
    mine = up[first + 1:first + 1 + len(groups)]
    for g, w in zip(mine, groups):
        assert name(g) == 'sn_sgd_mom_update_guarded_dev'
        assert w.endswith(', None)') and g == 'sn_sgd_mom_update_guarded_dev(' + w[len('sn_sgd_mom_update_dev('):-len('None)')] + \
            '0.5, tmp:float64:(8,), None)'
    assert up[first + 1 + len(groups):] == want[first + len(groups):]    # the refresh of the compute copies, as today


def test_guard_off_is_the_plain_update(monkeypatch):
    """set_grad_guard with nothing set: no guard, the committed trace of the update"""
    from sniper_amd.engine.executor import Executor
    init = Executor.__init__

    def init_then_off(self, *a, **kw):
        init(self, *a, **kw)
        self.set_grad_guard(clip_global_norm=1.0)
        self.set_grad_guard()
        assert self.guard is None
    monkeypatch.setattr(Executor, '__init__', init_then_off)
    assert trace(CASE, monkeypatch)[-1] == load()[CASE][-1]
    with pytest.raises(ValueError):
        Executor.set_grad_guard(object(), clip_gradient=0.0)
    with pytest.raises(ValueError):
        Executor.set_grad_guard(object(), clip_global_norm=float('nan'))


def test_guard_kernels_keep_registers_and_occupancy():
    """the compiler's resource remarks the build keeps beside the objects: the read stream and the guarded updates run eight waves per
    SIMD with nothing in scratch memory"""
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from test_kernel_resources import _resources
    found = 0
    for unit, frags in (('grad_guard', ('grad_guard_partial_kernel', 'grad_guard_finalize_kernel')),
                        ('nn_ops', ('sgd_guard_kernel', 'sgd_guard_vec4_kernel'))):
        res = _resources(unit)
        for frag in frags:
            hits = {k: v for k, v in res.items() if frag in k}
            assert len(hits) == 1, (frag, sorted(res))
            for name, r in hits.items():
                assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0 and r['Occupancy'] == 8, (name, r)
                found += 1
    assert found == 4


def test_header_declares_and_library_exports_the_guard():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import SniperHipError, lib
    L = lib()
    hdr = open(os.path.join(ROOT, 'include', 'sniper_hip.h')).read()
    dll = ctypes.CDLL(os.path.join(ROOT, 'sniper_amd', 'lib', 'libsniper_hip.so'))
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, hdr) and s in L.protos and hasattr(dll, s), s
    assert len(L.protos['sn_grad_guard'][1]) == 9 and len(L.protos['sn_sgd_mom_update_guarded_dev'][1]) == 11
    lim = (ctypes.c_int32 * 4)()
    L.call('sn_grad_guard_limits', lim)
    T, E, cap, nstate = (int(v) for v in lim)
    assert T % 64 == 0 and E % 4 == 0 and cap >= 256 and nstate == 8
    wsb = L.raw('sn_grad_guard_workspace_bytes')
    S = T * E
    assert wsb(1, 0) >= 16 and wsb(S * cap * 3, 0) >= 16 * cap and wsb(S * cap * 3, 0) == wsb(S * cap * 7, 0)
    assert wsb(S * 5, 2) >= 32 and wsb(S * 5, 0) >= 80
    # argument errors are reported before any launch (there is no device here: a launch would fail with another message)
    p = ctypes.c_void_p(16)
    for args in ((None, 4, p, 0.0, 0, 0, p, p, None), (p, -1, p, 0.0, 0, 0, p, p, None), (p, 4, p, -1.0, 0, 0, p, p, None),
                 (p, 4, p, float('nan'), 0, 0, p, p, None), (p, 4, p, 0.0, 0, -1, p, p, None), (p, 4, None, 0.0, 0, 0, p, p, None),
                 (p, 4, p, 0.0, 0, 0, None, p, None), (p, 4, p, 0.0, 0, 0, p, None, None), (ctypes.c_void_p(18), 4, p, 0.0, 0, 0, p, p, None)):
        with pytest.raises(SniperHipError) as e:
            L.call('sn_grad_guard', *args)
        assert 'sn_grad_guard' in str(e.value)
    for args in ((None, p, p, p, 4, p, 1.0, 1.0, 0.0, p, None), (p, p, p, p, -1, p, 1.0, 1.0, 0.0, p, None),
                 (p, p, p, p, 4, p, 1.0, 1.0, float('nan'), p, None), (p, p, p, p, 4, p, 1.0, 1.0, 0.0, None, None),
                 (p, p, p, p, 4, None, 1.0, 1.0, 0.0, p, None)):
        with pytest.raises(SniperHipError) as e:
            L.call('sn_sgd_mom_update_guarded_dev', *args)
        assert 'sn_sgd_mom_update_guarded_dev' in str(e.value)
