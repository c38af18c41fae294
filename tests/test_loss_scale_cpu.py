"""CPU: dynamic loss scaling without a device -- the restatement's policy on hand-written sequences, the options Module.init_optimizer
and Executor.set_loss_scale parse, optimizer_params and the symbols' grad_scale attributes under TRAIN.DYNAMIC_SCALE, the C-ABI calls a
scaled step issues (recorder of tests/golden/make_call_trace.py), the entry points in the header and the library with their argument
checks, the compiler's resource remarks for the new kernels, and the `.states` round trip."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import loss_scale_ref as ref  # noqa: E402
from make_call_trace import load, trace  # noqa: E402

SYMBOLS = ('sn_softmax_output_bwd_scaled', 'sn_fill_scaled_f32', 'sn_grad_guard_scaled', 'sn_aux_shadow')
POLICY = dict(growth_interval=3, growth_factor=2.0, backoff_factor=0.5, min_scale=1.0, max_scale=2.0 ** 24)


def _run(init, skips, **kw):
    p = dict(POLICY, **kw)
    ls = ref.new_ls(init)
    out = []
    for s in skips:
        ls = ref.policy(ls, bool(s), **p)
        out.append(ls.tolist())
    return out


def test_policy_on_hand_written_sequences():
    seq = _run(8.0, [0, 0, 0, 0, 1, 1, 0, 0, 0])
    assert [s[0] for s in seq] == [8, 8, 16, 16, 8, 4, 4, 4, 8]                 # scale for the next step
    assert [s[1] for s in seq] == [8, 8, 8, 16, 16, 8, 4, 4, 4]                 # scale the judged gradients carried
    assert [s[2] for s in seq] == [1, 2, 0, 1, 0, 0, 1, 2, 0]                   # clean steps since the scale changed
    assert seq[-1][3:] == [2.0, 2.0, 0.0, 0.0, 0.0]
    # growth_interval 0 never grows; a skipped step in between restarts the count
    assert [s[0] for s in _run(4.0, [0] * 7, growth_interval=0)] == [4.0] * 7
    assert [s[2] for s in _run(4.0, [0, 0, 1, 0, 0, 0], growth_interval=3)] == [1, 2, 0, 1, 2, 0]
    # clamps: held, counted, the clean count starts again
    top = _run(16.0, [0, 0], growth_interval=1, max_scale=16.0)
    assert [s[0] for s in top] == [16.0, 16.0] and top[-1][3:] == [0.0, 0.0, 2.0, 0.0, 0.0] and top[-1][2] == 0
    low = _run(1.0, [1, 1], min_scale=1.0)
    assert [s[0] for s in low] == [1.0, 1.0] and low[-1][3:] == [0.0, 0.0, 0.0, 2.0, 0.0]
    part = _run(2.0, [1], backoff_factor=0.25)          # cut short by min_scale: lowered AND held
    assert part[0][:2] == [1.0, 2.0] and part[0][3:] == [0.0, 1.0, 0.0, 1.0, 0.0]
    # factors of one: nothing moves, nothing is counted
    still = _run(4.0, [0, 1, 0], growth_interval=1, growth_factor=1.0, backoff_factor=1.0)
    assert [s[0] for s in still] == [4.0] * 3 and still[-1][3:] == [0.0] * 5
    # 2^30 reaches 2^0 in thirty back-offs
    down = _run(2.0 ** 30, [1] * 31, max_scale=2.0 ** 30)
    assert down[29][0] == 1.0 and down[29][4] == 30 and down[30][0] == 1.0 and down[30][4] == 30 and down[30][6] == 1


def test_restated_finalize_unscales_norm_and_coefficient():
    g = np.array([3.0, -4.0, 0.0, 12.0], np.float32) * np.float32(64)           # true gradient (3, -4, 0, 12): norm 13
    st, ls = ref.guard_scaled(g, -2.0, 13.0, np.zeros(8), ref.new_ls(64.0), **POLICY)
    assert st[0] == 26.0 and st[1] == (13.0 / (26.0 + 1e-6)) / 64 and st[2] == 0 and st[7] == 169.0 * 4096 and st[4] == 1
    assert ls.tolist() == [64.0, 64.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    g[1] = np.inf
    st, ls = ref.guard_scaled(g, 1.0, 0.0, st, ls, **POLICY)
    assert st[:7].tolist() == [np.sqrt(153.0), 1.0 / 64, 1.0, 1.0, 2.0, 1.0, 1.0] and ls.tolist() == [32.0, 64.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    sh = ref.Shadow([np.arange(3, dtype=np.float32), np.ones(2, np.float32)], total=9)
    sh.save()
    sh.vectors[0][:] = np.nan
    sh.restore([0, 0, 0.0])
    assert np.isnan(sh.vectors[0]).all()
    sh.restore([0, 0, 1.0])
    assert sh.vectors[0].tolist() == [0, 1, 2] and sh.shadow.tolist() == [0, 1, 2, 1, 1, 0, 0, 0, 0]


def _module():
    import sniper_amd.mx as mx
    return mx.mod.Module(mx.sym.Variable('x'), data_names=['x'], label_names=None)


BASE = {'learning_rate': 0.1, 'momentum': 0.9, 'wd': 1e-4, 'rescale_grad': 1.0, 'lr_scheduler': None}
BAD = [{'init_scale': 100.0}, {'init_scale': 0.0}, {'init_scale': -2.0}, {'init_scale': float('nan')}, {'init_scale': float('inf')},
       {'init_scale': 'big'}, {'init_scale': True}, {'growth_factor': 3.0}, {'growth_factor': 0.5}, {'backoff_factor': 0.3},
       {'backoff_factor': 2.0}, {'min_scale': 3.0}, {'max_scale': 1000.0}, {'min_scale': 4.0, 'max_scale': 2.0, 'init_scale': 2.0},
       {'init_scale': 2.0 ** 25}, {'init_scale': 0.5}, {'growth_interval': -1}, {'growth_interval': 2.5}, {'growth_interval': True},
       {'max_scale': 2.0 ** 128, 'init_scale': 2.0}, {'min_scale': 2.0 ** -127}]


def test_init_optimizer_parses_dynamic_loss_scale():
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    assert m.opt['loss_scale'] is None and m.opt['guard'] is False and m.loss_scale_state() is None
    for off in (None, False):
        m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=off))
        assert m.opt['loss_scale'] is None
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=True))
    assert m.opt['loss_scale'] == dict(init_scale=65536.0, growth_interval=2000, growth_factor=2.0, backoff_factor=0.5, min_scale=1.0,
                                       max_scale=2.0 ** 24, restore_aux=True)
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale={'init_scale': 128, 'growth_interval': 0,
                                                                                      'restore_aux': False}))
    assert m.opt['loss_scale']['init_scale'] == 128.0 and m.opt['loss_scale']['growth_interval'] == 0
    assert m.opt['loss_scale']['restore_aux'] is False and m.opt['loss_scale']['max_scale'] == 2.0 ** 24
    for bad in BAD + [{'restore_aux': 'yes'}, {'growth': 2.0}]:
        with pytest.raises(ValueError):
            _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=bad))
    for bad in ('on', 128, 2.0, ['init_scale']):
        with pytest.raises(ValueError):
            _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=bad))


def test_set_loss_scale_refuses_bad_values():
    from sniper_amd.engine.executor import Executor
    for bad in BAD:
        kw = dict(bad)
        init = kw.pop('init_scale', 128.0)
        with pytest.raises(ValueError):
            Executor.set_loss_scale(object(), init, **kw)


def test_optimizer_params_unfold_lr_and_wd():
    import inspect
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer, dynamic_loss_scale, optimizer_params
    cfg = cfgmod.res101_e2e(batch_images=2)
    tr = cfg.TRAIN
    assert tr.fp16 and tr.scale == 100.0 and not hasattr(tr, 'DYNAMIC_SCALE')
    op = optimizer_params(cfg)
    assert op['learning_rate'] == tr.lr / 100.0 and op['wd'] == tr.wd * 100.0 and 'dynamic_loss_scale' not in op
    assert dynamic_loss_scale(cfg) is None
    tr.DYNAMIC_SCALE = False
    assert optimizer_params(cfg) == op
    tr.DYNAMIC_SCALE = True
    op = optimizer_params(cfg)
    assert op['learning_rate'] == tr.lr and op['wd'] == tr.wd and op['rescale_grad'] == 1.0 and op['multi_precision'] is True
    assert op['dynamic_loss_scale'] == {'init_scale': 128.0}                   # the power of two nearest to 100 in log2
    assert op['clip_gradient'] is None and op['skip_nonfinite'] is False
    for scale, want in ((100.0, 128.0), (90.0, 64.0), (91.0, 128.0), (1.0, 1.0), (1024.0, 1024.0), (0.3, 0.25)):
        tr.scale = scale
        assert optimizer_params(cfg)['dynamic_loss_scale']['init_scale'] == want, scale
    tr.DYNAMIC_SCALE_INIT = 4096.0
    assert optimizer_params(cfg)['dynamic_loss_scale'] == {'init_scale': 4096.0}
    tr.DYNAMIC_SCALE = {'growth_interval': 500, 'init_scale': 256.0}
    assert optimizer_params(cfg)['dynamic_loss_scale'] == {'growth_interval': 500, 'init_scale': 256.0}
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=optimizer_params(cfg))
    assert m.opt['loss_scale']['init_scale'] == 256.0 and m.opt['loss_scale']['growth_interval'] == 500 and m.opt['lr'] == tr.lr
    assert inspect.signature(Trainer.__init__).parameters['dynamic_loss_scale'].default is None


def _grad_scales(name, preset, dynamic=None, fp16=True, scale=None):
    from sniper_amd import config as cfgmod
    from sniper_amd.mx import symbol as symmod
    symmod._counter().clear()
    cfg = getattr(cfgmod, preset)(batch_images=2)
    cfg.TRAIN.fp16 = fp16
    if scale is not None:
        cfg.TRAIN.scale = scale
    if dynamic is not None:
        cfg.TRAIN.DYNAMIC_SCALE = dynamic
    cls = getattr(importlib.import_module('sniper_amd.symbols.faster.' + name), name)
    sym = cls(momentum=0.995).get_symbol_rcnn(cfg)
    return {n.name: float(n.attrs['grad_scale']) for n in sym._topo() if 'grad_scale' in n.attrs}


def test_symbols_carry_no_scale_of_their_own_under_dynamic_scale():
    from test_frozen_bn_lowering import NETWORKS
    for name, (preset, _) in sorted(NETWORKS.items()):
        today = _grad_scales(name, preset)                      # the key unset: what the code produces without this feature
        assert len(today) >= 4 and today['rpn_cls_prob'] == 100.0, name
        assert _grad_scales(name, preset, dynamic=False) == today, name
        one = _grad_scales(name, preset, fp16=False)            # the key unset, no fp16: the attributes at scale 1
        assert one['rpn_cls_prob'] == 1.0
        for dyn in (True, {'growth_interval': 100}):
            got = _grad_scales(name, preset, dynamic=dyn)
            assert got == one, name                             # 1 x: the scale is not applied twice
            assert sorted(got) == sorted(today)
            for k in got:
                assert abs(got[k] * 100.0 - today[k]) <= 1e-12 * today[k], (name, k)
        assert _grad_scales(name, preset, dynamic=True, scale=512.0) == one, name


CASE = 'mobilenetv2_e2e/fix_bn=0'
_name = lambda line: line.split('(')[0]


def test_scaled_step_lowering(monkeypatch):
    """A scaled eager step: the save launch first in the forward, the _scaled loss calls in place of the plain ones (same buffers and
    scalars), sn_grad_guard_scaled, then the unchanged guarded updates, then the restore, then the refresh -- everything else is the
    committed trace."""
    from sniper_amd.engine.executor import Executor
    plain = load()[CASE]
    init = Executor.__init__
    made = []

    def scaled_init(self, *a, **kw):
        init(self, *a, **kw)
        self.set_loss_scale(128.0, growth_interval=7, max_scale=2.0 ** 20)
        made.append(self)
    monkeypatch.setattr(Executor, '__init__', scaled_init)
    got = trace(CASE, monkeypatch)
    ex = made[0]
    ls = ex.loss_scale
    assert ex.guard is not None and ex.guard['skip_nonfinite'] == 1 and ex._graph_fb is None and ex._graph_up is None
    assert ls['state'].dtype == torch.float64 and ls['state'].tolist() == [128.0] + [0.0] * 7
    bns = [s for s in ex.steps if type(s).__name__ == 'BatchNormStep' and not s.global_stats and not s.is_stem and s.folded_into is None]
    assert ls['n_aux'] == 2 * len(bns) > 0 and ls['table'].numel() == 16 * ls['n_aux']
    rec = ls['table'].numpy().view(np.dtype([('ptr', '<u8'), ('off', '<i4'), ('n', '<i4')]))
    want = [t for s in bns for t in (s.mean, s.var)]
    assert rec['ptr'].tolist() == [t.data_ptr() for t in want] and rec['n'].tolist() == [t.numel() for t in want]
    assert rec['off'].tolist() == np.concatenate([[0], np.cumsum(rec['n'])[:-1]]).tolist() and ls['shadow'].numel() >= int(rec['n'].sum())
    assert [p for p, _ in got] == [p for p, _ in plain]
    by = dict((p, (a, b)) for (p, a), (_, b) in zip(got, plain))
    for phase in ('setup', 'refresh'):
        assert by[phase][0] == by[phase][1]
    table = 'tmp:uint8:(%d,), %d, tmp:float32:(%d,)' % (16 * ls['n_aux'], ls['n_aux'], ls['shadow'].numel())
    fwd, fwd0 = by['forward']
    assert fwd[0] == 'sn_aux_shadow(%s, 0, None, None)' % table and fwd[1:] == fwd0
    bwd, bwd0 = by['backward']
    assert len(bwd) == len(bwd0)
    swapped = 0
    for a, b in zip(bwd, bwd0):
        if _name(b) == 'sn_softmax_output_bwd':
            assert a == 'sn_softmax_output_bwd_scaled(' + b[len('sn_softmax_output_bwd('):-len('None)')] + 'tmp:float64:(8,), None)'
            swapped += 1
        elif _name(b) == 'sn_ew_f32' and ', 4, ' in b and b.startswith('sn_ew_f32(None, None, '):
            m = re.match(r'sn_ew_f32\(None, None, (.*), (\d+), 4, ([^,]+), None\)$', b)
            assert a == 'sn_fill_scaled_f32(%s, %s, %s, tmp:float64:(8,), None)' % m.groups()
            swapped += 1
        else:
            assert a == b
    assert swapped == 4 and not [l for l in bwd if _name(l) == 'sn_softmax_output_bwd']
    up, up0 = by['update']
    first = [_name(l) for l in up0].index('sn_sgd_mom_update_dev')
    groups = [l for l in up0 if _name(l) == 'sn_sgd_mom_update_dev']
    n = ex.arena_grad.numel()
    assert up[:first] == up0[:first]
    args = up[first][len('sn_grad_guard_scaled('):-1]
    assert _name(up[first]) == 'sn_grad_guard_scaled' and args.startswith('par.')
    assert ':float32:(%d,), %d, tmp:float32:(4,), 0.0, 0, 7, 2.0, 0.5, 1.0, 1048576.0, tmp:uint8:' % (n, n) in args
    assert args.endswith('tmp:float64:(8,), tmp:float64:(8,), None')
    for g, w in zip(up[first + 1:first + 1 + len(groups)], groups):
        assert g == 'sn_sgd_mom_update_guarded_dev(' + w[len('sn_sgd_mom_update_dev('):-len('None)')] + '0.0, tmp:float64:(8,), None)'
    k = first + 1 + len(groups)
    assert up[k] == 'sn_aux_shadow(%s, 1, tmp:float64:(8,), None)' % table
    assert up[k + 1:] == up0[first + len(groups):]                        # the refresh of the compute copies, as today
    assert not [l for l in up if _name(l) in ('sn_grad_guard', 'sn_sgd_mom_update_dev')]


def test_split_backward_lowering_is_scaled_too(monkeypatch):
    from sniper_amd.engine.executor import Executor
    case = 'resnet_mx_101_e2e/split_backward'
    init = Executor.__init__

    def scaled_init(self, *a, **kw):
        init(self, *a, **kw)
        self.set_loss_scale(128.0, restore_aux=False)
    monkeypatch.setattr(Executor, '__init__', scaled_init)
    got, plain = trace(case, monkeypatch), load()[case]
    names = lambda phases: [_name(l) for _, lines in phases for l in lines]
    a, b = names(got), names(plain)
    assert 'sn_aux_shadow' not in a                                        # restore_aux=False: no table, no launches
    assert a.count('sn_softmax_output_bwd_scaled') == b.count('sn_softmax_output_bwd') > 0 and 'sn_softmax_output_bwd' not in a
    assert a.count('sn_fill_scaled_f32') > 0 and a.count('sn_grad_guard_scaled') == 1
    assert len(a) == len(b) + 1


def test_off_again_is_the_committed_trace(monkeypatch):
    from sniper_amd.engine.executor import Executor
    init = Executor.__init__

    def on_then_off(self, *a, **kw):
        init(self, *a, **kw)
        self.set_loss_scale(128.0)
        self.set_loss_scale(None)
        self.set_grad_guard()
        assert self.loss_scale is None and self.guard is None
    monkeypatch.setattr(Executor, '__init__', on_then_off)
    assert trace(CASE, monkeypatch) == load()[CASE]


def test_header_declares_and_library_exports_the_scaler():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import SniperHipError, lib
    L = lib()
    hdr = open(os.path.join(ROOT, 'include', 'sniper_hip.h')).read()
    dll = ctypes.CDLL(os.path.join(ROOT, 'sniper_amd', 'lib', 'libsniper_hip.so'))
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, hdr) and s in L.protos and hasattr(dll, s), s
    assert [len(L.protos[s][1]) for s in SYMBOLS] == [13, 5, 14, 6]
    assert L.protos['sn_grad_guard_scaled'][1][6:10] == [ctypes.c_double] * 4
    # existing entry points keep their signatures
    assert len(L.protos['sn_grad_guard'][1]) == 9 and len(L.protos['sn_softmax_output_bwd'][1]) == 12 and len(L.protos['sn_ew_f32'][1]) == 7
    # argument errors are reported before any launch (there is no device here: a launch would fail with another message)
    p = ctypes.c_void_p(16)
    ok = (p, 4, p, 0.0, 0, 3, 2.0, 0.5, 1.0, 2.0 ** 24, p, p, p, None)

    def but(**kw):
        names = L.protos['sn_grad_guard_scaled'][2]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    bad = [but(d_grad=None), but(n=-1), but(d_hyper=None), but(clip_global_norm=-1.0), but(clip_global_norm=float('nan')),
           but(max_blocks=-1), but(max_blocks=65536), but(d_ws=None), but(d_state=None), but(d_grad=ctypes.c_void_p(18)),
           but(d_ls=None), but(d_ls=ctypes.c_void_p(20)),
           but(growth_factor=3.0), but(growth_factor=0.5), but(growth_factor=0.0), but(growth_factor=float('inf')),
           but(backoff_factor=0.3), but(backoff_factor=2.0), but(backoff_factor=-0.5), but(backoff_factor=float('nan')),
           but(min_scale=3.0), but(min_scale=0.0), but(max_scale=1000.0), but(min_scale=4.0, max_scale=2.0),
           but(max_scale=2.0 ** 128), but(min_scale=2.0 ** -127), but(growth_interval=-1)]
    for args in bad:
        with pytest.raises(SniperHipError) as e:
            L.call('sn_grad_guard_scaled', *args)
        assert 'sn_grad_guard_scaled' in str(e.value), args
    for args in ((None, p, p, 4, 3, 1, -1.0, 1, 1.0, 0, p, p, None), (p, p, p, 4, 3, 1, -1.0, 1, 1.0, 0, p, None, None),
                 (p, p, p, 4, 3, 1, -1.0, 1, 1.0, 0, None, p, None), (p, p, p, 0, 3, 1, -1.0, 1, 1.0, 0, p, p, None),
                 (p, p, p, 4, 3, 1, -1.0, 1, 1.0, 0, p, ctypes.c_void_p(12), None)):
        with pytest.raises(SniperHipError) as e:
            L.call('sn_softmax_output_bwd_scaled', *args)
        assert 'sn_softmax_output_bwd_scaled' in str(e.value)
    for args in ((None, 4, 1.0, p, None), (p, 0, 1.0, p, None), (p, 4, 1.0, None, None), (p, 4, 1.0, ctypes.c_void_p(12), None)):
        with pytest.raises(SniperHipError) as e:
            L.call('sn_fill_scaled_f32', *args)
        assert 'sn_fill_scaled_f32' in str(e.value)
    for args in ((None, 3, p, 0, None, None), (p, 3, None, 0, None, None), (p, 3, p, 1, None, None), (p, 3, p, 2, p, None),
                 (p, -1, p, 0, None, None), (ctypes.c_void_p(12), 3, p, 0, None, None), (p, 3, ctypes.c_void_p(18), 0, None, None)):
        with pytest.raises(SniperHipError) as e:
            L.call('sn_aux_shadow', *args)
        assert 'sn_aux_shadow' in str(e.value)
    assert L.call('sn_aux_shadow', None, 0, None, 1, None, None) == 0          # an empty table: no launch


def test_scaler_kernels_use_no_scratch():
    """the compiler's resource remarks the build keeps beside the objects: nothing in scratch memory, no spills -- the new kernels,
    and the softmax gradients and the guard's two kernels that now share their statements with them"""
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from test_kernel_resources import _resources
    found = 0
    for unit, frags in (('loss_scale', ('softmax_bwd_scaled_kernel', 'softmax_rows_bwd_scaled_kernel', 'fill_scaled_kernel',
                                        'grad_guard_scaled_finalize_kernel', 'aux_shadow_kernel')),
                        ('nn_ops', ('softmax_bwd_kernel', 'softmax_rows_bwd_kernel')),
                        ('grad_guard', ('grad_guard_partial_kernel', 'grad_guard_finalize_kernel'))):
        res = _resources(unit)
        for frag in frags:
            hits = {k: v for k, v in res.items() if frag in k}
            assert len(hits) == 1, (frag, sorted(res))
            for name, r in hits.items():
                assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
                found += 1
    assert found == 9
    assert len(_resources('loss_scale')) == 5                                 # no second copy of the guard's partial pass in this unit


def _tiny_module():
    """an unbound Module around one CPU executor of a two-layer graph: what save_checkpoint / load_optimizer_states touch"""
    import sniper_amd.mx as mx
    from sniper_amd.engine.executor import Executor
    from sniper_amd.mx import symbol as symmod
    symmod._counter().clear()
    x = mx.sym.FullyConnected(data=mx.sym.Variable('data'), num_hidden=8, name='fc')
    sym = mx.sym.SoftmaxOutput(data=x, label=mx.sym.Variable('label'), name='prob', grad_scale=1.0)
    m = mx.mod.Module(sym, data_names=['data'], label_names=['label'])
    ex = Executor(sym, dict(data=(4, 16), label=(4,)), True, [], device=torch.device('cpu'))
    m.exe, m._exes, m._device, m.for_training, m.binded = ex, {'only': ex}, torch.device('cpu'), True, True
    return m


def test_init_optimizer_turns_the_scaler_on_and_off_again(monkeypatch):
    from sniper_amd import hip
    monkeypatch.setattr(hip, 'call', lambda *a: 0)
    monkeypatch.setattr(hip, 'stream', lambda: None)
    m = _tiny_module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=True, clip_global_norm=5.0))
    ex = m.exe
    assert ex.loss_scale is not None and ex.guard['skip_nonfinite'] == 1 and ex.guard['clip_global_norm'] == 5.0
    assert m.loss_scale_state()['scale'] == 65536.0
    with pytest.raises(ValueError):
        ex.set_loss_scale(2.0 ** 25)                     # above max_scale: refused, and the scaler stays as it was
    assert ex.loss_scale['state'][0] == 65536.0
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, skip_nonfinite=True))
    assert ex.loss_scale is None and ex.guard is not None and m.loss_scale_state() is None
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    assert ex.loss_scale is None and ex.guard is None


def test_states_round_trip(tmp_path, monkeypatch):
    from sniper_amd import hip
    monkeypatch.setattr(hip, 'call', lambda *a: 0)
    monkeypatch.setattr(hip, 'stream', lambda: None)
    dyn = {'init_scale': 128.0, 'growth_interval': 5}
    m = _tiny_module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=dyn))
    assert m.loss_scale_state() == dict(scale=128.0, scale_used=0.0, clean=0, growths=0, backoffs=0, held_max=0, held_min=0)
    assert m.grad_guard_state()['steps'] == 0 and m.exe.guard['skip_nonfinite'] == 1
    m.exe.loss_scale['state'][0], m.exe.loss_scale['state'][2] = 32.0, 3.0          # as after some back-offs and three clean steps
    m.exe.arena_mom.copy_(torch.arange(m.exe.arena_mom.numel(), dtype=torch.float32))
    m.exe.num_update = 17
    prefix = str(tmp_path / 'ck')
    m.save_checkpoint(prefix, 2, save_optimizer_states=True)
    st = torch.load(prefix + '-0002.states')
    assert st['loss_scale'] == 32.0 and st['clean'] == 3 and st['num_update'] == 17
    r = _tiny_module()
    r.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=dyn))
    r.load_optimizer_states(prefix + '-0002.states')
    assert r.loss_scale_state()['scale'] == 32.0 and r.loss_scale_state()['clean'] == 3 and r.exe.num_update == 17
    assert torch.equal(r.exe.arena_mom, m.exe.arena_mom)
    r._guard_exe(r.exe)                                  # an executor bound later starts at the resumed scale too
    assert r.loss_scale_state()['scale'] == 32.0 and r.loss_scale_state()['clean'] == 3
    # a file without the two keys (the scaler off when it was written) loads as before and leaves the scale alone
    s = _tiny_module()
    s.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    s.exe.num_update = 5
    s.save_checkpoint(prefix, 3, save_optimizer_states=True)
    assert sorted(torch.load(prefix + '-0003.states')) == ['momentum', 'num_update']
    r.load_optimizer_states(prefix + '-0003.states')
    assert r.loss_scale_state()['scale'] == 32.0 and r.exe.num_update == 5
    # and a file with them loads into a run without the scaler
    s.load_optimizer_states(prefix + '-0002.states')
    assert s.loss_scale_state() is None and s.exe.num_update == 17
    torch.save(dict(st, loss_scale=100.0), prefix + '-0004.states')
    with pytest.raises(ValueError):
        r.load_optimizer_states(prefix + '-0004.states')
