"""-m gpu: moving-statistics BatchNorm inside a training graph (fix_bn).  sn_bn_frozen_backward against the formulas in
float64, sn_bn_global_scale_shift_batch against the per-layer entry, and the R101 fix_bn network end to end: teacher-forced
parity with oracle/graph_cpu.py, hipGraph replay against eager steps, bitwise reproducibility, and the launches a step issues."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import assert_close, dev  # noqa: E402

EPS = 2e-5


def _hip():
    from sniper_amd import hip
    return hip


def _td(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).to(dt)


def _rows(t, ps):
    """(M, C) fp16 -> the same values as rows of a (M, ps) buffer (pixel stride ps >= C; the padding holds a sentinel)"""
    M, C = t.shape
    if ps == C:
        return t.contiguous()
    buf = torch.full((M, ps), 9.0, dtype=t.dtype, device=t.device)
    buf[:, :C] = t
    return buf


class _Case(object):
    """Inputs as test_bn_apply_and_backward_blocks_equal_the_separate_launches draws them, and the float64 reference."""

    def __init__(self, M, C, act, ps, fix_gamma=False):
        hip = _hip()
        self.M, self.C, self.act, self.ps = M, C, act, ps
        rs = np.random.RandomState(M + C + act + ps)
        x = _td(rs.standard_normal((M, C)) * 1.5 + 0.3, torch.float16)
        dy = _td(rs.standard_normal((M, C)), torch.float16)
        acc = _td(rs.standard_normal((M, C)), torch.float16)
        self.gamma = None if fix_gamma else _td(rs.uniform(0.5, 1.5, C))
        self.beta, self.mean, self.var = _td(rs.standard_normal(C) * 0.1), _td(rs.standard_normal(C) * 0.2 + 0.3), _td(rs.uniform(0.5, 1.5, C))
        self.scale, self.shift = torch.empty(C, device=dev()), torch.empty(C, device=dev())
        hip.call('sn_bn_global_scale_shift', self.gamma, self.beta, self.mean, self.var, C, EPS, self.scale, self.shift, hip.stream())
        d = lambda t: t.double()
        g64 = d(self.gamma) if self.gamma is not None else torch.ones(C, dtype=torch.float64, device=dev())
        self.invstd = 1.0 / torch.sqrt(d(self.var) + EPS)
        sc64 = g64 * self.invstd
        sh64 = d(self.beta) - d(self.mean) * sc64
        assert_close(self.scale.cpu().numpy(), sc64.cpu().numpy(), 1e-6, 1e-7, 'scale')
        assert_close(self.shift.cpu().numpy(), sh64.cpu().numpy(), 1e-6, 1e-6, 'shift')
        # elements within 1e-3 of an activation edge: the kernel decides them on its own fp32 rounding of x * scale + shift.  They
        # are left out of the dx comparison and out of the sums on BOTH sides (their dy is zero in what the kernel reads)
        yf = d(x) * sc64 + sh64
        keep = torch.ones_like(yf, dtype=torch.bool)
        ok = keep
        if act:
            keep = (yf.abs() > 1e-3) & ((yf - 6).abs() > 1e-3) if act == 2 else yf.abs() > 1e-3
            ok = (yf >= 0) & (yf <= 6) if act == 2 else yf > 0
        self.left_out = 1.0 - float(keep.double().mean())
        dy = torch.where(keep, dy, torch.zeros_like(dy))
        g = d(dy) * ok
        self.keep = keep
        self.want_db = g.sum(0)
        self.want_dg = (g * (d(x) - d(self.mean))).sum(0) * self.invstd
        self.want_dx = sc64 * g
        self.acc64 = d(acc)
        self.x, self.dy, self.acc = _rows(x, ps), _rows(dy, ps), _rows(acc, ps)
        self.ws = torch.empty(hip.query('sn_bn_workspace_bytes', M, C), dtype=torch.uint8, device=dev())

    def run(self, want_dx, want_par, accumulate, arena=(0.0, 0.0)):
        """-> (dx (M, C) or None, dgamma or None, dbeta or None); the padding of a strided dx must stay untouched"""
        hip = _hip()
        M, C, ps = self.M, self.C, self.ps
        dx = torch.full((M, ps), 7.0, dtype=torch.float16, device=dev()) if want_dx else None
        dg = torch.full((C,), arena[0], dtype=torch.float32, device=dev()) if want_par and self.gamma is not None else None
        db = torch.full((C,), arena[1], dtype=torch.float32, device=dev()) if want_par else None
        hip.call('sn_bn_frozen_backward', self.dy, self.x, self.acc if (accumulate and want_dx) else None, dx, M, C, ps, ps, ps, ps,
                 self.scale, self.shift, self.mean, self.var, EPS, self.act, self.ws if want_par else None, dg, db, hip.stream())
        torch.cuda.synchronize()
        if dx is not None and ps > C:
            assert bool((dx[:, C:] == 7.0).all()), 'dx wrote beyond its C channels'
        return (dx[:, :C] if dx is not None else None), dg, db


# (M, C, act, pixel stride): the six launch shapes of the C2 step (2 x 20 chips), a ragged ReLU6 one, two channel slabs, no
# activation, a strided source, and a fix_gamma layer
CASES = [(81920, 128, 1, 128), (81920, 512, 1, 512), (20480, 256, 1, 256), (20480, 1024, 1, 1024), (20480, 512, 1, 512),
         (20480, 2048, 1, 2048), (5000, 192, 2, 192), (18, 2560, 1, 2560), (3000, 72, 0, 72), (3000, 72, 1, 104), (2048, 64, 1, 64)]


@pytest.mark.parametrize('M,C,act,ps', CASES)
def test_bn_frozen_backward_vs_float64(M, C, act, ps):
    """sn_bn_frozen_backward in its three modes, with and without `accumulate`, onto a non-zero gradient arena, against
    dx = scale * g (+ acc), dbeta = sum g, dgamma = sum g * (x - moving_mean) * invstd in float64.  Tolerances: dx 1e-2 relative /
    1e-2 of the largest value (fp16 output), dbeta / dgamma 1e-5 relative / 1e-4 absolute against float64 sums of the same masked
    fp16 inputs.  Parameter-only and dx-only calls are BIT-equal to the combined call, and two combined calls to each other."""
    case = _Case(M, C, act, ps, fix_gamma=(M == 2048))
    print('left out near an activation edge: %.4f %%' % (100 * case.left_out))
    assert case.left_out <= 2e-3
    keep = case.keep
    dg0, db0 = None, None
    for accumulate in (False, True):
        want = case.want_dx + (case.acc64 if accumulate else 0)
        dx, dg, db = case.run(True, True, accumulate, arena=(0.5, -0.5))            # dx and parameter gradients
        dx_b, dg_b, db_b = case.run(True, True, accumulate, arena=(0.5, -0.5))      # ... twice: bit-equal
        dx_only, _, _ = case.run(True, False, accumulate)                           # dx only
        _, dg_p, db_p = case.run(False, True, accumulate)                           # parameter gradients only, zero arena
        assert torch.equal(dx, dx_b) and torch.equal(db, db_b) and (dg is None or torch.equal(dg, dg_b))
        assert torch.equal(dx, dx_only), float((dx.float() - dx_only.float()).abs().max())
        assert torch.equal(db, db_p - 0.5) and (dg is None or torch.equal(dg, dg_p + 0.5))
        err = float(((dx.double() - want).abs() * keep).max())
        print('accumulate %d: max |dx error| %.3e of max |dx| %.3e' % (accumulate, err, float(want.abs().max())))
        assert_close(dx.double()[keep].cpu().numpy(), want[keep].cpu().numpy(), 1e-2, 1e-2 * float(want.abs().max()), 'dx')
        print('max |dbeta error| %.3e (max |dbeta| %.3e)' % (float((db_p.double() - case.want_db).abs().max()), float(case.want_db.abs().max())))
        assert_close(db_p.cpu().numpy(), case.want_db.cpu().numpy(), 1e-5, 1e-4, 'dbeta')
        if dg_p is not None:
            print('max |dgamma error| %.3e (max |dgamma| %.3e)' % (float((dg_p.double() - case.want_dg).abs().max()),
                                                                  float(case.want_dg.abs().max())))
            assert_close(dg_p.cpu().numpy(), case.want_dg.cpu().numpy(), 1e-5, 1e-4, 'dgamma')
        if dg0 is not None or db0 is not None:      # the parameter gradients do not depend on `accumulate`
            assert torch.equal(db_p, db0) and (dg_p is None or torch.equal(dg_p, dg0))
        dg0, db0 = dg_p, db_p


def test_bn_frozen_backward_rejects_bad_arguments():
    hip = _hip()
    from sniper_amd.hip import SniperHipError
    t = torch.zeros((16, 8), dtype=torch.float16, device=dev())
    v = torch.ones(8, device=dev())
    with pytest.raises(SniperHipError):       # nothing asked for
        hip.call('sn_bn_frozen_backward', t, t, None, None, 16, 8, 8, 8, 8, 8, v, v, v, v, EPS, 1, None, None, None, hip.stream())
    with pytest.raises(SniperHipError):       # parameter gradients without a workspace
        hip.call('sn_bn_frozen_backward', t, t, None, None, 16, 8, 8, 8, 8, 8, v, v, v, v, EPS, 1, None, v, v, hip.stream())
    with pytest.raises(SniperHipError):       # C not a multiple of 8
        hip.call('sn_bn_frozen_backward', t, t, None, t, 16, 4, 8, 8, 8, 8, v, v, v, v, EPS, 1, None, None, None, hip.stream())


def test_bn_global_scale_shift_batch_equals_per_layer():
    hip = _hip()
    rs = np.random.RandomState(6)
    widths = [8, 64, 72, 256, 2560, 24, 1024, 2048, 512, 96, 8]
    layers = []
    for k, C in enumerate(widths):
        gamma = None if k % 3 == 1 else _td(rs.uniform(0.5, 1.5, C))
        layers.append((gamma, _td(rs.standard_normal(C)), _td(rs.standard_normal(C)), _td(rs.uniform(1e-3, 2.0, C)), C,
                       (2e-5, 1e-3)[k % 2]))
    rec = np.zeros(len(layers), dtype=np.dtype([('gamma', '<u8'), ('beta', '<u8'), ('mean', '<u8'), ('var', '<u8'), ('scale', '<u8'),
                                                ('shift', '<u8'), ('C', '<i4'), ('eps', '<f4')]))
    assert rec.dtype.itemsize == 56
    single, batched = [], []
    for k, (g, b, m, v, C, eps) in enumerate(layers):
        sc, sh = torch.full((C + 8,), 7.0, device=dev()), torch.full((C + 8,), 7.0, device=dev())
        hip.call('sn_bn_global_scale_shift', g, b, m, v, C, eps, sc, sh, hip.stream())
        single.append((sc, sh))
        sc, sh = torch.full((C + 8,), 7.0, device=dev()), torch.full((C + 8,), 7.0, device=dev())
        batched.append((sc, sh))
        rec[k] = (0 if g is None else g.data_ptr(), b.data_ptr(), m.data_ptr(), v.data_ptr(), sc.data_ptr(), sh.data_ptr(), C, eps)
    desc = torch.from_numpy(rec.view(np.uint8).copy()).to(dev())
    hip.call('sn_bn_global_scale_shift_batch', desc, len(layers), hip.stream())
    torch.cuda.synchronize()
    for (g, b, m, v, C, eps), (s0, h0), (s1, h1) in zip(layers, single, batched):
        assert torch.equal(s0, s1) and torch.equal(h0, h1), C
        assert bool((s1[C:] == 7.0).all()) and bool((h1[C:] == 7.0).all()), C
        g64 = 1.0 if g is None else g.double()
        assert_close(s1[:C].cpu().numpy(), (g64 / torch.sqrt(v.double() + eps)).cpu().numpy(), 1e-6, 1e-7, 'scale C=%d' % C)


# ---------------------------------------------------------------------------------------------------------------------
# the R101 fix_bn network
# ---------------------------------------------------------------------------------------------------------------------
A, F = 21, 32


def _r101(B, fix_bn, graphs='0'):
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.symbols.faster import resnet_mx_101_e2e as rn
    from sniper_amd.train import fixed_param_names
    cfg = cfgmod.res101_e2e(batch_images=B)
    sym = rn.resnet_mx_101_e2e(momentum=0.995, fix_bn=fix_bn).get_symbol_rcnn(cfg)
    shapes = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, A * F * F),
                  bbox_target=(B, 4 * A, F, F), bbox_weight=(B, 4 * A, F, F), gt_boxes=(B, 100, 5))
    old = os.environ.get('SNIPER_HIP_GRAPHS')
    os.environ['SNIPER_HIP_GRAPHS'] = graphs
    try:
        ex = Executor(sym, shapes, True, fixed_param_names(cfg, sym))
    finally:
        if old is None:
            os.environ.pop('SNIPER_HIP_GRAPHS', None)
        else:
            os.environ['SNIPER_HIP_GRAPHS'] = old
    return sym, shapes, ex


def _r101_params(sym, shapes, rs):
    from test_gpu_engine import _init_params
    P, AUX = _init_params(sym, shapes, rs, bn_gamma=(0.5, 1.0), bn_beta=(-0.2, 0.4))
    P['bn_data_gamma'][:] = 1.0
    AUX['bn_data_moving_mean'][:] = 0.0
    AUX['bn_data_moving_var'][:] = 1.0 - 2e-5      # bn_data == identity: the image stays fp16-representable
    P['bn_data_beta'][:] = 0.0
    return P, AUX


def _batch_statistics(B, P, AUX, feed):
    """Moving statistics as a pretrained trunk would bring them (random ones normalise nothing: the first gradients of the 100-layer
    network are ~1e7 and it diverges at any learning rate worth testing): the batch statistics of one training forward of the
    fix_bn=False network, momentum 0."""
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.symbols.faster import resnet_mx_101_e2e as rn
    from sniper_amd.train import fixed_param_names
    cfg = cfgmod.res101_e2e(batch_images=B)
    sym = rn.resnet_mx_101_e2e(momentum=0.0).get_symbol_rcnn(cfg)
    shapes = {k: tuple(v.shape) for k, v in feed.items()}
    os.environ['SNIPER_HIP_GRAPHS'] = '0'
    try:
        ex = Executor(sym, shapes, True, fixed_param_names(cfg, sym))
    finally:
        os.environ.pop('SNIPER_HIP_GRAPHS', None)
    ex.set_params(P, AUX)
    ex.forward(feed, is_train=True)
    torch.cuda.synchronize()
    aux = ex.get_params()[1]
    assert all(np.isfinite(v).all() for v in aux.values())
    return aux


def test_r101_fix_bn_network_parity_vs_cpu_reference_ops():
    """resnet_mx_101_e2e(fix_bn=True) at 2 chips through the teacher-forced comparison of tests/test_gpu_engine.py, that file's
    tolerances for the same network; every gradient the fix_bn=False graph has is checked (gamma / beta of stages 2 - 4 included),
    and the moving statistics come out bit-equal to what was set."""
    from test_gpu_engine import _forced_parity, _train_inputs
    B = 2
    _, _, ex0 = _r101(B, False)
    n_expected = sum(1 for p in ex0.params.values() if p.trainable)
    names0 = sorted(n for n, p in ex0.params.items() if p.trainable)
    del ex0
    sym, shapes, ex = _r101(B, True)
    assert sorted(n for n, p in ex.params.items() if p.trainable) == names0
    rs = np.random.RandomState(12)
    P, AUX = _r101_params(sym, shapes, rs)
    inp = _train_inputs(rs, B, A, F)
    checked, _ = _forced_parity(sym, ex, P, AUX, inp, tol_fwd=2e-3, tol_grad=1e-2)
    assert checked == n_expected and checked >= 250
    assert sum(1 for n in names0 if n.endswith(('_gamma', '_beta')) and n.startswith(('stage2', 'stage3', 'stage4'))) == 180
    for name, t in ex.aux.items():
        assert np.array_equal(t.cpu().numpy(), AUX[name]), name


def test_r101_fix_bn_graph_replay_matches_eager():
    """Five steps under hipGraph replay against five eager steps (the manner and tolerance of test_hip_graph_replay_matches_eager).
    The refreshed scale / shift belong to the captured optimizer pass: after the last step every trainable moving-statistics layer
    holds exactly the scale / shift of its CURRENT gamma / beta."""
    hip = _hip()
    B = 2
    rs = np.random.RandomState(5)
    results, P, AUX, feeds = [], None, None, None
    for graphs in ('0', '1'):
        sym, shapes, ex = _r101(B, True, graphs)
        assert ex.use_graphs == (graphs == '1')
        if P is None:
            from test_gpu_engine import _train_inputs
            P, AUX = _r101_params(sym, shapes, rs)
            feeds = [_train_inputs(rs, B, A, F) for _ in range(5)]
            AUX = _batch_statistics(B, P, AUX, feeds[0])
        ex.set_params(P, AUX)
        outs = []
        for i, feed in enumerate(feeds):
            o = ex.forward_backward(feed)
            outs.append([t.clone() for t in o])
            print('graphs %s step %d: max |gradient| %.4g' % (graphs, i, float(ex.arena_grad.abs().max())))
            # (gradients carry the static loss scale of 100: at most 2/3 of the config's own learning rate; a changing learning
            # rate must reach the replayed graph)
            ex.update(lr=2e-5 * (i + 1), wd=1e-3, momentum=0.9)
            print('graphs %s step %d: max |parameter| %.4g' % (graphs, i, float(ex.arena_master.abs().max())))
        torch.cuda.synchronize()
        if graphs == '1':
            assert ex._graph_fb is not None and ex._graph_up is not None, 'hipGraph capture did not happen'
        assert bool(torch.isfinite(ex.arena_master).all()), 'training diverged'
        layers = [s for s in ex.steps if type(s).__name__ == 'BatchNormStep' and s.batched_refresh()]
        assert len(layers) == 90
        for s in layers:
            sc, sh = torch.empty_like(s.scale), torch.empty_like(s.shift)
            hip.call('sn_bn_global_scale_shift', s.gamma.master, s.beta.master, s.mean, s.var, s.C, s.eps, sc, sh, hip.stream())
            assert torch.equal(sc, s.scale) and torch.equal(sh, s.shift), 'stale scale / shift in ' + s.node.name
            assert not torch.equal(s.gamma.master.cpu(), torch.from_numpy(P[s.gamma.name])), s.node.name + ': gamma did not train'
        for name, t in ex.aux.items():
            assert np.array_equal(t.cpu().numpy(), AUX[name]), name
        results.append((outs, {k: p.master.clone() for k, p in ex.params.items()}))
        del ex
    (oe, pe), (og, pg) = results
    for a, b in zip(oe, og):
        for x, y in zip(a, b):
            assert torch.isfinite(y).all()
            assert_close(y.cpu().numpy(), x.cpu().numpy(), 2e-2, 2e-2 * float(x.abs().max()) + 1e-6, 'graph vs eager outputs')
    for k in pe:
        assert_close(pg[k].cpu().numpy(), pe[k].cpu().numpy(), 2e-2, 2e-2 * float(pe[k].abs().max()) + 1e-6, 'graph vs eager ' + k)


# The synthetic runs start from RANDOM weights (no pretrained file), with statistics calibrated on one batch that cannot follow the
# weights afterwards: at the config's own learning rate (1.5e-4 on loss-scaled gradients) such a network leaves its statistics
# behind within two updates and overflows fp16.  fix_bn is a fine-tuning mode; the tests train at a fine-tuning rate.
_SGD = {'learning_rate': 2e-5, 'momentum': 0.9, 'wd': 0.01}


def test_fix_bn_training_is_bitwise_reproducible():
    """Two fresh runs of three Trainer(fix_bn=True) steps (two eager, one replay): every output and parameter bit for bit."""
    from sniper_amd.train import Trainer
    runs = []
    for rep in range(2):
        tr = Trainer(batch_images=2, n_images=4, seed=11, fix_bn=True)
        tr.mod.init_optimizer(optimizer='sgd', optimizer_params=_SGD)
        rec = []
        for step in range(3):
            outs = tr.step()
            torch.cuda.synchronize()
            rec.append([o.asnumpy().copy() for o in outs])
            assert all(np.isfinite(o).all() for o in rec[-1]), 'step %d is not finite' % step       # (and nothing more is launched)
        rec.append(tr.mod.exe.arena_master.detach().cpu().numpy().copy())
        runs.append(rec)
        del tr
    a, b = runs
    for step in range(3):
        for k, (u, v) in enumerate(zip(a[step], b[step])):
            assert np.isfinite(u).all() and np.array_equal(u, v), 'output %d differs at step %d' % (k, step)
    assert np.array_equal(a[3], b[3]), 'parameters differ after 3 steps'


@pytest.mark.parametrize('preset', ['res101_e2e', 'res101_e2e_mask', 'rfcn'])
def test_trainer_fix_bn_trains_under_graph_replay(preset):
    """Trainer(fix_bn=True) on the R101, mask and R-FCN networks: six steps on a repeated batch (two eager, then hipGraph
    replays), finite outputs, a falling RPN loss, and moving statistics that never move."""
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer
    if preset == 'rfcn':
        cfg = cfgmod.res101_e2e(batch_images=2)
        cfg.symbol = 'resnet_mx_101_e2e_rfcn'
    else:
        cfg = getattr(cfgmod, preset)(batch_images=2)
    tr = Trainer(batch_images=2, n_images=4, seed=0, cfg=cfg, fix_bn=True)
    ex = tr.mod.exe
    assert sum(1 for s in ex.steps if type(s).__name__ == 'BatchNormStep' and s.batched_refresh()) == 90
    b = tr.batch

    def rpn_ce(outs):
        p = outs[0].asnumpy()
        lab = b.label[0].asnumpy().reshape(p.shape[0], -1)
        p = p.reshape(p.shape[0], 2, -1)
        m = lab != -1
        sel = np.where(lab == 1, p[:, 1], p[:, 0])
        return float(-np.log(sel[m] + 1e-12).mean())

    aux0 = {k: t.clone() for k, t in ex.aux.items()}
    tr.mod.forward(b, is_train=True)
    l0 = rpn_ce(tr.mod.get_outputs())
    tr.mod.init_optimizer(optimizer='sgd', optimizer_params=_SGD)
    for k in range(6):
        outs = tr.step(b)
        torch.cuda.synchronize()
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'step %d is not finite' % k     # (and nothing more is launched)
    assert ex._graph_fb is not None and ex._graph_up is not None, 'hipGraph capture did not happen'
    for o in outs:
        assert np.isfinite(o.asnumpy()).all()
    l1 = rpn_ce(outs)
    print('%s: RPN cross entropy %.5f -> %.5f' % (preset, l0, l1))
    assert np.isfinite(l1) and l1 < l0, (l0, l1)
    for k, t in aux0.items():
        assert torch.equal(t, ex.aux[k]), k


def test_fix_bn_step_launches(monkeypatch):
    """One eager training step of the fix_bn graph, counted at sniper_amd.hip.call: no batch statistics, no finalize, no
    statistics epilogue and no batch-statistics backward anywhere; one sn_bn_frozen_backward per trainable-stage layer; one
    sn_bn_global_scale_shift_batch in the optimizer pass and no per-layer sn_bn_global_scale_shift in the whole step."""
    from sniper_amd import hip
    from sniper_amd.train import Trainer
    monkeypatch.setenv('SNIPER_HIP_GRAPHS', '0')
    tr = Trainer(batch_images=2, n_images=4, seed=0, fix_bn=True)
    calls, real = [], hip.call

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(hip, 'call', counting)
    tr.mod.forward_backward(tr.batch)
    n_fb = len(calls)
    tr.mod.update()
    torch.cuda.synchronize()
    monkeypatch.setattr(hip, 'call', real)
    count = lambda n, part=None: (calls if part is None else part).count(n)
    for name in ('sn_bn_stats', 'sn_bn_finalize', 'sn_bn_finalize_blocks', 'sn_bn_apply_blocks', 'sn_conv_fwd_stats', 'sn_bn_backward',
                 'sn_bn_backward_blocks', 'sn_conv_dgrad_bn', 'sn_bn_global_scale_shift'):
        assert count(name) == 0, (name, count(name))
    assert count('sn_bn_frozen_backward') == 90
    assert count('sn_bn_apply') == 101 - 1 - 7           # every layer but bn_data (stem packing) and the 7 folded frozen ones
    assert count('sn_bn_global_scale_shift_batch', calls[n_fb:]) == 1 and count('sn_bn_global_scale_shift_batch', calls[:n_fb]) == 0
