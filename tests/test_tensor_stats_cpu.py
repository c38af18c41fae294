"""CPU: the per-tensor statistics without a device -- the numpy restatement against direct numpy on hand-written vectors, the planner
through ctypes, the entry points in the header and the library, mx.mon.Monitor on a stand-in executor, the options, and the C-ABI calls
of an optimizer pass with the skip report on and off (recorder of tests/golden/make_call_trace.py)."""
import ctypes
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import tensor_stats_ref as ref  # noqa: E402
from make_call_trace import load, trace  # noqa: E402

SYMBOLS = ('sn_tensor_stats_limits', 'sn_tensor_stats_plan', 'sn_tensor_stats_plan_bytes', 'sn_tensor_stats_workspace_bytes',
           'sn_tensor_stats')


def _lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib
    return lib()


def _limits():
    out = (ctypes.c_int32 * 6)()
    _lib().call('sn_tensor_stats_limits', out)
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def test_restatement_on_hand_written_vectors():
    x = np.array([3, np.inf, -4, np.nan, -0.0, 0], np.float32)
    assert ref.record(x, 4).tolist() == [25.0, -1.0, 2.0, 1.0, 4.0, 2.0, 6.0, 0.0]
    assert ref.record(x, 1 << 20).tolist() == [25.0, -1.0, 2.0, 1.0, 4.0, 2.0, 6.0, 0.0]
    assert ref.record(np.zeros(0, np.float32), 4).tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0]
    assert ref.record(np.array([np.nan], np.float32), 4).tolist() == [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    h = np.array([65504, -2.0 ** -24, -np.inf, 1.5], np.float16)
    assert ref.record(h, 2).tolist() == [65504.0 ** 2 + 2.0 ** -48 + 2.25, 65504.0 - 2.0 ** -24 + 1.5, 1.0, 2.0, 65504.0, 0.0, 4.0, 0.0]
    big = np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max], np.float32)
    r = ref.record(big, 8)
    assert r[0] == 2.0 * float(big[0]) ** 2 and r[1] == 0.0 and r[2] == 0 and r[4] == float(big[0])
    # against direct numpy on random data: the fields that do not depend on the order, and the sums within one rounding per addition
    rs = np.random.RandomState(0)
    v = rs.standard_normal(1000).astype(np.float32)
    v[[7, 500]] = np.nan, -np.inf
    v[[3, 4]] = 0.0, -0.0
    r = ref.record(v, 64)
    ok = np.isfinite(v)
    d = v[ok].astype(np.float64)
    assert r[2] == 2 and r[3] == 7 and r[4] == np.abs(d).max() and r[5] == 2 and r[6] == 1000
    assert abs(r[0] - np.sum(d * d)) <= 1000 * 2.0 ** -53 * np.sum(d * d) and abs(r[1] - np.sum(d)) <= 1000 * 2.0 ** -53 * np.sum(np.abs(d))


def test_restated_output_header_monitor_value_and_report():
    arena = np.full(40, np.nan, np.float32)
    segs = [(2, 3), (8, 0), (10, 4), (20, 6)]
    arena[2:5] = 1, 2, 2
    arena[10:14] = 1, np.inf, 0, -1
    arena[20:26] = 3, np.inf, -4, np.nan, -0.0, 0
    out = ref.stats(arena, segs, 4, step=41)
    assert out.shape == (5, 8)
    assert out[0].tolist() == [1.0, 41.0, 4.0, 2.0, 2.0, 0.0, 0.0, 0.0]
    assert out[1].tolist() == [9.0, 5.0, 0.0, -1.0, 2.0, 0.0, 3.0, 0.0]
    assert out[2].tolist() == [0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0]
    assert out[4].tolist() == [25.0, -1.0, 2.0, 1.0, 4.0, 2.0, 6.0, 0.0]
    assert ref.monitor_value(out[1]) == 3.0 / np.sqrt(3.0)
    assert np.isnan(ref.monitor_value(out[2])) and np.isnan(ref.monitor_value(out[3]))
    assert ref.stats(arena, segs[:2], 4)[0].tolist() == [1.0, 0.0, 2.0, 0.0, -1.0, 0.0, 0.0, 0.0]
    names = ['a', 'b', 'c', 'd']
    rep = ref.report(out, names)
    assert rep['step'] == 41 and [t['name'] for t in rep['tensors']] == ['c', 'd']
    assert rep['tensors'][1] == {'name': 'd', 'nonfinite': 2, 'first_index': 1, 'max_abs': 4.0, 'norm': 5.0, 'zeros': 2, 'numel': 6}
    assert ref.report(np.zeros((5, 8)), names) is None
    # the production code states the same two rules
    from sniper_amd.mx.module import Module
    from sniper_amd.mx.mon import default_stat
    assert Module._report_dict(out, names) == rep
    for r in out[1:]:
        a, b = default_stat(r), ref.monitor_value(r)
        assert (np.isnan(a) and np.isnan(b)) or a == b


# ------------------------------------------------------------------------------------------------
# the planner
# ------------------------------------------------------------------------------------------------
def _plan(segs):
    """-> (items [(off, toff, len, tensor)], tensors [(n, first, count)]) through the C ABI, into a buffer of exactly the size asked for"""
    L = _lib()
    T = len(segs)
    seg = np.ascontiguousarray(np.asarray(segs, np.int64).reshape(T, 2))
    n_items = ctypes.c_int32(-1)
    L.call('sn_tensor_stats_plan', seg.ctypes.data, T, None, 0, ctypes.byref(n_items))
    n_items = n_items.value
    nbytes = L.raw('sn_tensor_stats_plan_bytes')(T, n_items)
    assert nbytes == 32 * n_items + 16 * T
    buf = np.zeros(nbytes // 8 + 1, np.int64)
    buf[-1] = 0x5a5a5a5a
    again = ctypes.c_int32(-1)
    L.call('sn_tensor_stats_plan', seg.ctypes.data, T, buf.ctypes.data, nbytes, ctypes.byref(again))
    assert again.value == n_items and buf[-1] == 0x5a5a5a5a
    raw = buf[:-1].view(np.uint8)
    items = raw[:32 * n_items].view(np.dtype([('off', '<i8'), ('toff', '<i8'), ('len', '<i4'), ('tensor', '<i4'), ('pad', '<i8')]))
    tens = raw[32 * n_items:].view(np.dtype([('n', '<i8'), ('first', '<i4'), ('count', '<i4')]))
    assert L.raw('sn_tensor_stats_workspace_bytes')(T, n_items) >= 64 * n_items
    return items, tens


def _check_cover(segs):
    """every element of every segment in exactly one item of its own tensor; a tensor's items ascending and consecutive"""
    _, C, _, _, _, _ = _limits()
    items, tens = _plan(segs)
    assert len(tens) == len(segs) and not items['pad'].any()
    seg = np.asarray(segs, np.int64).reshape(len(segs), 2)
    off, n = seg[:, 0], seg[:, 1]
    count = -(-n // C)
    first = np.cumsum(count) - count
    assert np.array_equal(tens['n'], n) and np.array_equal(tens['count'], count) and np.array_equal(tens['first'], first)
    assert len(items) == count.sum()
    # item k of the plan is chunk j of tensor t: tensor after tensor, a tensor's chunks ascending, whole but for the last, back to back
    t = np.repeat(np.arange(len(segs)), count)
    j = np.arange(len(items)) - first[t]
    assert np.array_equal(items['tensor'], t) and np.array_equal(items['toff'], j * C) and np.array_equal(items['off'], off[t] + j * C)
    assert np.array_equal(items['len'], np.minimum(C, n[t] - j * C)) and (items['len'] >= 1).all()
    assert np.array_equal(np.bincount(t, weights=items['len'], minlength=len(segs)).astype(np.int64), n)      # every element once
    return len(items)


def test_planner_covers_every_element_once():
    S, C, maxT, rec, S16, cap = _limits()
    assert rec == 8 and S % 1024 == 0 and S16 == 2 * S and C % S16 == 0 and maxT >= 1000 and cap >= 256
    assert _check_cover([]) == 0                                          # T = 0
    assert _check_cover([(0, 0), (7, 0), (7, 0)]) == 0                    # n = 0: no item
    assert _check_cover([(5, 1)]) == 1
    assert _check_cover([(3, 100 * C + 17)]) == 101
    assert _check_cover([(999 - t, 1) for t in range(1000)]) == 1000      # any order
    lens = [0, 1, 3, 4, 7, 8, 15, 16, S - 1, S, S + 1, C - 1, C, C + 1, 3 * C + 5]
    segs, off = [], 0
    for k, n in enumerate(lens):
        off += 1 + k % 9
        segs.append((off, n))
        off += n
    assert _check_cover(segs) == sum(-(-n // C) for n in lens)
    assert _check_cover([(8 * t, t % 8) for t in range(maxT)]) == maxT - maxT // 8
    assert _check_cover([(0, 10), (10, 5)]) == 2                          # touching is not overlapping


def test_planner_refuses_bad_tables():
    from sniper_amd._lib import SniperHipError
    L = _lib()
    _, C, maxT, _, _, _ = _limits()
    n = ctypes.c_int32(0)

    def plan(segs, T=None):
        seg = np.ascontiguousarray(np.asarray(segs, np.int64).reshape(-1, 2))
        L.call('sn_tensor_stats_plan', seg.ctypes.data, len(seg) if T is None else T, None, 0, ctypes.byref(n))
    for segs, word in (([(0, 10), (20, 5), (9, 3)], 'overlap'), ([(0, 10), (0, 10)], 'overlap'), ([(4, 2 * C), (C, 1)], 'overlap'),
                       ([(-1, 4)], 'negative'), ([(0, -4)], 'negative'), ([(2 ** 63 - 3, 5)], 'overflows')):
        with pytest.raises(SniperHipError) as e:
            plan(segs)
        assert 'sn_tensor_stats_plan' in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(SniperHipError) as e:
        plan([(8 * t, 1) for t in range(maxT + 1)])
    assert 'outside' in str(e.value)
    with pytest.raises(SniperHipError):
        plan([(0, 1)], T=-1)
    with pytest.raises(SniperHipError):
        L.call('sn_tensor_stats_plan', None, 2, None, 0, ctypes.byref(n))
    seg = np.array([[0, 3 * C]], np.int64)
    buf = np.zeros(64, np.int64)
    with pytest.raises(SniperHipError) as e:                              # a plan buffer one item short
        L.call('sn_tensor_stats_plan', seg.ctypes.data, 1, buf.ctypes.data, 32 * 2 + 16, ctypes.byref(n))
    assert 'needed' in str(e.value)


def test_header_declares_and_library_exports_the_entry_points():
    from sniper_amd._lib import SniperHipError
    L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'sniper_hip.h')).read()
    dll = ctypes.CDLL(os.path.join(ROOT, 'sniper_amd', 'lib', 'libsniper_hip.so'))
    for s in SYMBOLS:
        assert re.search(r'\b%s\s*\(' % s, hdr) and s in L.protos and hasattr(dll, s), s
    assert len(L.protos['sn_tensor_stats'][1]) == 11 and L.protos['sn_tensor_stats'][2][-1] == 'stream'
    wsb = L.raw('sn_tensor_stats_workspace_bytes')
    assert wsb(0, 0) > 0 and wsb(3, 10) >= 640 and wsb(-1, 0) == 0 and wsb(1, -1) == 0
    # argument errors are reported before any launch (there is no device here: a launch would fail with another message)
    p = ctypes.c_void_p(64)
    good = [p, 1, p, 1, 1, 0, p, 0, p, p, None]
    for pos, bad in ((0, None), (2, None), (8, None), (9, None), (1, 2), (1, -1), (4, -1), (4, 1 << 20), (3, -1), (5, -1), (5, 65536),
                     (0, ctypes.c_void_p(66)), (9, ctypes.c_void_p(68)), (6, ctypes.c_void_p(68))):
        args = list(good)
        args[pos] = bad
        with pytest.raises(SniperHipError) as e:
            L.call('sn_tensor_stats', *args)
        assert 'sn_tensor_stats' in str(e.value), (pos, bad)
    with pytest.raises(SniperHipError) as e:                              # only_if_skipped without the guard's state
        L.call('sn_tensor_stats', p, 1, p, 1, 1, 0, None, 1, p, p, None)
    assert 'only_if_skipped' in str(e.value)
    with pytest.raises(SniperHipError):                                   # fp16 needs 2-byte, fp32 4-byte alignment
        L.call('sn_tensor_stats', ctypes.c_void_p(65), 0, p, 1, 1, 0, None, 0, p, p, None)


# ------------------------------------------------------------------------------------------------
# mx.mon.Monitor on a stand-in executor (CPU tensors, the restatement in place of the launches)
# ------------------------------------------------------------------------------------------------
class FakeExe(object):
    def __init__(self):
        rs = np.random.RandomState(1)
        self.names = ['fc_weight', 'fc_bias', 'conv_weight']
        self.t = {w: [torch.from_numpy(rs.standard_normal(n).astype(np.float32)) for n in (12, 4, 30)] for w in ('weight', 'grad', 'mom')}
        self.t['grad'][2][5] = float('inf')
        self.out = torch.from_numpy(rs.standard_normal((2, 3)).astype(np.float32))
        self.launches = []

    def _match(self, pattern, suffix):
        return [k for k, n in enumerate(self.names) if re.match(pattern, n + suffix)]

    def tensor_stats(self, which, pattern=None, suffix=''):
        self.launches.append(which)
        ks = self._match(pattern, suffix)
        arena = np.concatenate([self.t[which][k].numpy() for k in ks]) if ks else np.zeros(0, np.float32)
        segs, off = [], 0
        for k in ks:
            segs.append((off, self.t[which][k].numel()))
            off += segs[-1][1]
        return torch.from_numpy(ref.stats(arena, segs, 8)), [self.names[k] for k in ks]

    def output_stats(self, pattern=None):
        if not re.match(pattern, 'cls_prob_output'):
            return []
        self.launches.append('output')
        return [('cls_prob_output', torch.from_numpy(ref.stats(self.out.numpy().ravel(), [(0, 6)], 8)))]

    def stat_views(self, pattern=None):
        rows = []
        for which, suffix in (('weight', ''), ('grad', '_grad'), ('mom', '_mom')):
            rows += [(self.names[k] + suffix, self.t[which][k]) for k in self._match(pattern, suffix)]
        if re.match(pattern, 'cls_prob_output'):
            rows.append(('cls_prob_output', self.out))
        return rows


def test_monitor_interval_pattern_sort_and_values():
    import sniper_amd.mx as mx
    assert mx.mon is mx.monitor and mx.mon.Monitor is not None
    ex = FakeExe()
    mon = mx.mon.Monitor(3)
    mon.install(ex)
    armed = []
    for batch in range(7):
        mon.tic()
        n = len(ex.launches)
        rows = mon.toc()
        armed.append(bool(rows))
        if rows:
            assert all(r[0] == batch + 1 for r in rows) and len(ex.launches) == n + 4
        else:
            assert len(ex.launches) == n                  # an un-armed batch asks the executor for nothing
        assert mon.toc() == []                            # toc disarms
    assert armed == [True, False, False, True, False, False, True]
    mon.tic()                                             # (batch 8: not armed)
    mon.tic()
    mon.tic()
    rows = mon.toc()
    names = [r[1] for r in rows]
    assert names == ['fc_weight', 'fc_bias', 'conv_weight', 'fc_weight_grad', 'fc_bias_grad', 'conv_weight_grad',
                     'fc_weight_mom', 'fc_bias_mom', 'conv_weight_mom', 'cls_prob_output']
    assert all(isinstance(r[2], str) for r in rows)
    val = dict((r[1], float(r[2])) for r in rows)
    for which, suffix in (('weight', ''), ('grad', '_grad'), ('mom', '_mom')):
        for k, n in enumerate(ex.names):
            x = ex.t[which][k].numpy().astype(np.float64)
            want = np.sqrt(np.sum(x * x)) / np.sqrt(x.size)
            got = val[n + suffix]
            if n + suffix == 'conv_weight_grad':
                assert np.isnan(got) and not np.isfinite(want)   # a non-finite element: the norm is not finite, the row says nan
            else:
                assert abs(got - want) <= x.size * 2.0 ** -53 * want
    # pattern and sort
    mon = mx.mon.Monitor(1, pattern='.*(weight|weight_grad)$', sort=True)
    mon.install(ex)
    mon.tic()
    assert [r[1] for r in mon.toc()] == ['conv_weight', 'conv_weight_grad', 'fc_weight', 'fc_weight_grad']
    mon = mx.mon.Monitor(1, pattern='.*(weight|weight_grad)$')
    mon.install(ex)
    mon.extra_rows.append(lambda: [('loss_scale', 128.0)])
    mon.tic()
    assert [r[1] for r in mon.toc()] == ['fc_weight', 'conv_weight', 'fc_weight_grad', 'conv_weight_grad', 'loss_scale']
    for bad in (dict(interval=0), dict(interval=1.5), dict(interval=True), dict(interval=2, pattern='('), dict(interval=2, pattern=None),
                dict(interval=2, stat_func=3)):
        with pytest.raises(ValueError):
            mx.mon.Monitor(**bad)


def test_monitor_toc_print_row_format_and_stat_func(caplog):
    import sniper_amd.mx as mx
    ex = FakeExe()
    seen = []

    def stat(x):
        seen.append(x)
        return mx.nd.array(np.abs(x.asnumpy()).max().reshape(1))
    mon = mx.mon.Monitor(2, stat_func=stat, pattern='fc_.*|cls_prob_output')
    mon.install(ex)
    with caplog.at_level(logging.INFO):
        mon.tic()
        mon.toc_print()
        mon.tic()
        mon.toc_print()
    lines = [r.getMessage() for r in caplog.records if r.getMessage().startswith('Batch:')]
    names = ['fc_weight', 'fc_bias', 'fc_weight_grad', 'fc_bias_grad', 'fc_weight_mom', 'fc_bias_mom', 'cls_prob_output']
    assert len(lines) == len(names) == len(seen) and ex.launches == []     # the slow path: one call of stat_func per tensor, no launch
    assert all(isinstance(x, mx.nd.NDArray) for x in seen)
    want = float(np.abs(ex.t['weight'][0].numpy()).max())
    assert lines[0] == 'Batch: {:7d} {:30s} {:s}'.format(1, 'fc_weight', str(want))
    assert [ln.split()[2] for ln in lines] == names and all(ln.startswith('Batch:       1 ') for ln in lines)


# ------------------------------------------------------------------------------------------------
# options
# ------------------------------------------------------------------------------------------------
def _module():
    import sniper_amd.mx as mx
    return mx.mod.Module(mx.sym.Variable('x'), data_names=['x'], label_names=None)


BASE = {'learning_rate': 0.1, 'momentum': 0.9, 'wd': 1e-4, 'rescale_grad': 1.0, 'lr_scheduler': None}


def test_options_are_parsed_and_bad_values_refused(monkeypatch):
    monkeypatch.delenv('SNIPER_SKIP_REPORT', raising=False)
    monkeypatch.delenv('SNIPER_MONITOR', raising=False)
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))
    assert m.opt['skip_report'] is False and m.skip_report() is None
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, skip_nonfinite=True, skip_report=True))
    assert m.opt['skip_report'] is True
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, dynamic_loss_scale=True, skip_report=True))
    assert m.opt['skip_report'] is True
    for bad in (dict(skip_report=True), dict(skip_report=True, clip_global_norm=1.0), dict(skip_nonfinite=True, skip_report='yes'),
                dict(skip_nonfinite=True, skip_report=2)):
        with pytest.raises(ValueError):
            _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, **bad))
    monkeypatch.setenv('SNIPER_SKIP_REPORT', '1')
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, skip_nonfinite=True))
    assert m.opt['skip_report'] is True
    m.init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, skip_nonfinite=True, skip_report=False))     # the key wins
    assert m.opt['skip_report'] is False
    with pytest.raises(ValueError):
        _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE))                                   # nothing skips
    monkeypatch.setenv('SNIPER_SKIP_REPORT', 'on')
    with pytest.raises(ValueError):
        _module().init_optimizer(optimizer='sgd', optimizer_params=dict(BASE, skip_nonfinite=True))
    monkeypatch.delenv('SNIPER_SKIP_REPORT')
    # SNIPER_MONITOR=<interval>[:<regex>]
    from sniper_amd.mx.module import Module
    from sniper_amd.mx.mon import parse_monitor_env
    assert Module._monitor_from_env() is None
    assert parse_monitor_env('50') == (50, '.*') and parse_monitor_env(' 2:.*(weight|bias)_grad$') == (2, '.*(weight|bias)_grad$')
    assert parse_monitor_env('3:a:b') == (3, 'a:b')
    monkeypatch.setenv('SNIPER_MONITOR', '4:fc.*')
    mon = Module._monitor_from_env()
    assert (mon.interval, mon.pattern, mon.stat_func, mon.sort) == (4, 'fc.*', None, False)
    for bad in ('x', '0', '-2', '1.5', '2:(', ':abc'):
        monkeypatch.setenv('SNIPER_MONITOR', bad)
        with pytest.raises(ValueError):
            Module._monitor_from_env()


def test_config_keys_and_trainer_arguments():
    import inspect
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer, monitor_from_config, optimizer_params
    cfg = cfgmod.res101_e2e(batch_images=2)
    assert optimizer_params(cfg)['skip_report'] is None and monitor_from_config(cfg) is None
    cfg.TRAIN.SKIP_REPORT, cfg.TRAIN.SKIP_NONFINITE = True, True
    op = optimizer_params(cfg)
    assert op['skip_report'] is True
    m = _module()
    m.init_optimizer(optimizer='sgd', optimizer_params=op)
    assert m.opt['skip_report'] is True
    cfg.TRAIN.MONITOR_INTERVAL = 5
    mon = monitor_from_config(cfg)
    assert (mon.interval, mon.pattern) == (5, '.*')
    cfg.TRAIN.MONITOR_PATTERN = '.*_grad$'
    assert monitor_from_config(cfg).pattern == '.*_grad$'
    for key, bad in (('MONITOR_INTERVAL', 0), ('MONITOR_INTERVAL', 'often'), ('MONITOR_PATTERN', '(')):
        c = cfgmod.res101_e2e(batch_images=2)
        c.TRAIN.MONITOR_INTERVAL = 5
        setattr(c.TRAIN, key, bad)
        with pytest.raises(ValueError):
            monitor_from_config(c)
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig['skip_report'].default is False and sig['monitor'].default is None
    for kw in (dict(skip_report='yes'), dict(skip_report=True), dict(monitor=5)):     # (skip_report without anything that skips)
        with pytest.raises(ValueError):
            Trainer(batch_images=2, n_images=4, **kw)


def test_monitor_rows_end_with_the_loss_scale_the_gradients_carry():
    """no scale: no row; a static scale the caller folded into lr / wd: that one; a dynamic scale: the one the last optimizer pass left
    as 'used', and inside an accumulation window (no pass since the forward) or before the first pass the current one"""
    m = _module()

    class Exe(object):
        loss_scale = None
    m.exe = Exe()
    m.opt = {'accumulate': 1}
    assert m._monitor_scale_row() == []
    m.static_loss_scale = 100.0
    assert m._monitor_scale_row() == [('loss_scale', 100.0)]
    Exe.loss_scale = {'state': torch.tensor([256.0, 128.0, 0, 0, 1, 0, 0, 0], dtype=torch.float64)}
    assert m._monitor_scale_row() == [('loss_scale', 128.0)]
    m.opt, m._accum_pending = {'accumulate': 2}, 1
    assert m._monitor_scale_row() == [('loss_scale', 256.0)]
    m._accum_pending = 0
    assert m._monitor_scale_row() == [('loss_scale', 128.0)]
    Exe.loss_scale['state'][1] = 0.0
    assert m._monitor_scale_row() == [('loss_scale', 256.0)]


def test_set_skip_report_needs_a_guard_that_skips():
    from sniper_amd.engine.executor import Executor

    class Stub(object):
        guard = None
        skip_report = 'x'
        _graph_up = 'graph'
    s = Stub()
    with pytest.raises(ValueError):
        Executor.set_skip_report(s, True)
    s.guard = {'skip_nonfinite': 0}
    with pytest.raises(ValueError):
        Executor.set_skip_report(s, True)
    with pytest.raises(ValueError):
        Executor.set_skip_report(s, 1)
    assert s._graph_up == 'graph'
    Executor.set_skip_report(s, False)
    assert s.skip_report is None and s._graph_up is None


# ------------------------------------------------------------------------------------------------
# the C-ABI calls of an optimizer pass
# ------------------------------------------------------------------------------------------------
CASE = 'mobilenetv2_e2e/fix_bn=0'
name = lambda line: line.split('(')[0]


def _traced(monkeypatch, after_init):
    from sniper_amd.engine.executor import Executor
    init = Executor.__init__
    made = []

    def wrapped(self, *a, **kw):
        init(self, *a, **kw)
        after_init(self)
        made.append(self)
    monkeypatch.setattr(Executor, '__init__', wrapped)
    return trace(CASE, monkeypatch), made[0]


def test_report_on_adds_exactly_one_call_behind_the_guard(monkeypatch):
    def on(ex):
        ex.set_grad_guard(skip_nonfinite=True)
        ex.set_skip_report(True)
    got, ex = _traced(monkeypatch, on)
    plain = load()[CASE]
    for (phase, a), (_, b) in zip(got[:-1], plain[:-1]):
        assert a == b, phase                                  # set-up, forward, backward: untouched
    up = got[-1][1]
    names = [name(l) for l in up]
    assert names.count('sn_tensor_stats') == 1 and names.count('sn_grad_guard') == 1
    k = names.index('sn_tensor_stats')
    assert names[k - 1] == 'sn_grad_guard' and names[k + 1] == 'sn_sgd_mom_update_guarded_dev'
    tab = ex.skip_report['table']
    T, n = tab['T'], ex.arena_grad.numel()
    assert T == len([p for p in ex.params.values() if p.trainable]) > 10 and tab is ex.stat_tables['grad'] is ex.stat_tables['mom']
    assert tab['names'] == [p.name for p in sorted((p for p in ex.params.values() if p.trainable), key=lambda p: p.offset)]
    assert [tuple(s) for s in tab['segs']] == [(ex.params[k].offset, ex.params[k].numel) for k in tab['names']]
    args = up[k][len('sn_tensor_stats('):-1]
    assert args.startswith('par.') and ':float32:(%d,), 1, tmp:int64:' % n in args
    assert args.endswith(', %d, %d, 0, tmp:float64:(8,), 1, tmp:uint8:(%d,), tmp:float64:(%d, 8), None' % (tab['n_items'], T, tab['ws'].numel(), 1 + T))
    assert tuple(ex.skip_report['out'].shape) == (1 + T, 8) and not ex.skip_report['out'].any()
    # a filtered table is a cached sub-table, in arena order
    sub = ex.stat_table('.*weight_grad$', '_grad')
    assert sub is ex.stat_table('.*weight_grad$', '_grad') and sub['names'] == [k for k in tab['names'] if k.endswith('weight')]
    assert 0 < sub['T'] < T
    with pytest.raises(ValueError):
        ex.tensor_stats('activations')


def test_report_off_and_an_unarmed_monitor_batch_are_the_guarded_pass_of_today(monkeypatch):
    import sniper_amd.mx as mx

    def guarded(ex):
        ex.set_grad_guard(skip_nonfinite=True)
    want, _ = _traced(monkeypatch, guarded)
    want = [[p, list(lines)] for p, lines in want]
    monkeypatch.undo()

    def on_then_off(ex):
        ex.set_grad_guard(skip_nonfinite=True)
        ex.set_skip_report(True)
        ex.set_skip_report(False)
        assert ex.skip_report is None
    got, ex = _traced(monkeypatch, on_then_off)
    assert got == want
    assert 'sn_tensor_stats' not in [name(l) for _, lines in got for l in lines]
    # the guard turned off takes the report with it
    ex.set_skip_report(True)
    ex.set_grad_guard()
    assert ex.guard is None and ex.skip_report is None
    # a Monitor on this executor: the armed batch issues one launch pair per arena and one per head, the next batch none
    lines = got[-1][1]
    mon = mx.mon.Monitor(2, pattern='.*(weight|weight_grad)$|.*_output$')
    mon.install(ex)
    mon.tic()
    n0 = len(lines)
    rows = mon.toc()
    added = [name(l) for l in lines[n0:]]
    heads = len(ex.outputs)
    assert added.count('sn_tensor_stats') == 2 + heads and len(rows) == 2 * ex.stat_table('.*(weight|weight_grad)$|.*_output$')['T'] + heads
    assert [l for l in lines[n0:] if name(l) == 'sn_tensor_stats'][1].startswith('sn_tensor_stats(par.')
    ex.update(0.01, 1e-4, 0.9, 1.0)
    mon.tic()
    n1 = len(lines)
    assert mon.toc() == [] and len(lines) == n1
