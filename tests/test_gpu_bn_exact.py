"""-m gpu: the BatchNorm family (and its unfused siblings sn_ew_f16 / sn_clip_f16) against float64 references ON THE BITS
(bn_exact_util.py; DESIGN.md "Exact BatchNorm tests").  Integer operands and power-of-two coefficients make every sum exact and
put 9-14 % of the elements exactly on an activation edge, so a row lost or counted twice at a row-block seam, an 8-channel chunk
of the second slab not written, an edge element masked the wrong way or `accumulate` read after the store is a mismatch, not noise
under a tolerance.  M walks the seams of bn_grid for every channel count (bn_exact_util.seams); every operand -- the per-channel
vectors and the workspace included -- lives in a guarded buffer (NaN around inputs, a sentinel around outputs that must survive the
launch) at dense and padded pitches and as a channel slice; `accumulate` is absent, a buffer of its own, and ALIASED to dx, which
is how Executor.grad_slot hands it to every backward kernel of a training step."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_exact_util as bx  # noqa: E402
from bn_exact_util import Guarded, kinds  # noqa: E402

F16, F32 = torch.float16, torch.float32
EPS, SMALL = 2e-5, 1 << 20            # SMALL: elements up to which a case runs every activation x accumulate mode
NBLKS = (1, 31, 32, 33, 512, 513, 1280)      # the 32-lane walk of bn_sum_partials: one lane, a ragged / whole / one-over round, 16+ rounds
ACC_MODES = ('none', 'own', 'aliased')


def _hip():
    from sniper_amd import hip
    return hip


def _in(values, kind='dense', dtype=F16):
    values = np.asarray(values)
    if values.ndim == 1:
        values = values[None]
    return Guarded(values.shape[0], values.shape[1], kind, dtype=dtype, values=values)


def _out(rows, C, kind='dense', dtype=F16):
    return Guarded(rows, C, kind, dtype=dtype)


def _inout(values, kind='dense', dtype=F16):
    """an operand a launch reads AND writes: the values inside, the sentinel around them"""
    values = np.asarray(values)
    if values.ndim == 1:
        values = values[None]
    g = Guarded(values.shape[0], values.shape[1], kind, dtype=dtype)
    g.view.copy_(torch.from_numpy(np.array(values, dtype=np.float64)).to(g.flat.device))
    return g


def _ws(M, C):
    """the workspace as a guarded output: a launch that writes past sn_bn_workspace_bytes meets the sentinel"""
    nbytes = _hip().query('sn_bn_workspace_bytes', M, C)
    assert nbytes == bx.workspace_bytes(M, C), (M, C, nbytes)
    return Guarded(1, nbytes // 4, 'dense', dtype=F32)


def _clean(what, *bufs):
    for b in bufs:
        if b is not None:
            assert b.untouched(), '%s: the launch wrote outside a %d x %d operand (pitch %d, offset %d)' % (what, b.rows, b.C, b.pitch, b.offset)


def _ok(msgs):
    msgs = [m for m in msgs if m]
    assert not msgs, '\n'.join(msgs)


def _acts(i, M, C):
    return bx.ACTS if M * C <= SMALL else (bx.ACTS[i % 3],)


# ---------------------------------------------------------------------------------------------------------------- sn_bn_apply
GRID_STRIDE = (8200, 2056)          # 8200 * 257 chunks > 8192 blocks x 256 threads: the second trip of the elementwise kernels' loop


def _grid_stride_operands(lo, hi):
    M, C = GRID_STRIDE
    rs = np.random.RandomState(bx.case_seed(GRID_STRIDE, 1))
    return rs.randint(lo, hi + 1, size=(M, C)).astype(np.float32)


@pytest.mark.parametrize('C', bx.C_EDGES)
def test_bn_apply_exact(C):
    """y = act(x * scale + shift) with the test's coefficients: multiples of 0.5, every one an fp16 value; the clamp at exactly 6
    and the zero of relu included.  Out of place at rotating pitches, and in place (y == x)."""
    hip = _hip()
    n = bx.Counts()
    for i, (M, _) in enumerate(bx.cases(C)):
        q = bx.problem(M, C)
        x = _in(q.x, kinds(i, 0))
        sc, sh = _in(q.scale, kinds(i, 1), F32), _in(q.shift, kinds(i, 2), F32)
        pre = q.x * q.scale + q.shift
        for act in bx.ACTS:
            what = 'sn_bn_apply act %d M %d C %d' % (act, M, C)
            want = bx.apply_ref(q, act)
            y = _out(M, C, kinds(i, 3 + act))
            hip.call('sn_bn_apply', x.view, y.view, M, C, x.pitch, y.pitch, sc.view, sh.view, act, hip.stream())
            _ok([bx.compare_exact(y.result(), want, what)])
            _clean(what, y)
            n.add('launches')
            if act in _acts(i, M, C):
                io = _inout(q.x, kinds(i, 2 + act))
                hip.call('sn_bn_apply', io.view, io.view, M, C, io.pitch, io.pitch, sc.view, sh.view, act, hip.stream())
                _ok([bx.compare_exact(io.result(), want, what + ' in place')])
                _clean(what + ' in place', io)
                n.add('launches')
                n.add('in_place')
            n.add('edge_elements', bx.edge_mask(pre, act).sum())
        n.add('cases')
    if C == GRID_STRIDE[1]:
        M = GRID_STRIDE[0]
        xv = _grid_stride_operands(-4, 4)
        q = bx.problem(1024, C)
        sc, sh = _in(q.scale, 'dense', F32), _in(q.shift, 'slice', F32)
        x, y = _in(xv, 'dense'), _out(M, C, '+8')
        hip.call('sn_bn_apply', x.view, y.view, M, C, x.pitch, y.pitch, sc.view, sh.view, 2, hip.stream())
        want = np.clip(xv * q.scale.astype(np.float32) + q.shift.astype(np.float32), 0, 6)
        _ok([bx.compare_exact(y.result(), want, 'sn_bn_apply grid-stride')])
        _clean('sn_bn_apply grid-stride', y)
        n.add('grid_stride')
    n['M'], n['seams'] = list(bx.m_edges(C)), sorted(bx.seams(C))
    n.log('bn_apply C %d' % C)
    assert n['cases'] == len(bx.cases(C)) >= 8 and n['launches'] >= 4 * n['cases'] and n['in_place'] >= n['cases']
    assert n['edge_elements'] >= 0.05 * 2 * sum(M * C for M, _ in bx.cases(C))


# ------------------------------------------------------------------------------------------------- sn_bn_stats + sn_bn_finalize
def _forward_variant(i):
    """(momentum, running statistics start at zero): 0.9 onto a non-zero state (two roundings: within 1 ulp), 0.9 onto zero and 0.5
    (exact updates: on the bits)"""
    return ((0.9, False), (0.9, True), (0.5, False))[i % 3]


class _FwdOut(object):
    def __init__(self, i, C, r, k=0):
        self.sc, self.sh = _out(1, C, kinds(i, k), F32), _out(1, C, kinds(i, k + 1), F32)
        self.sm, self.si = _out(1, C, kinds(i, k + 2), F32), _out(1, C, kinds(i, k + 3), F32)
        self.rm, self.rv = _inout(r.run_mean0, kinds(i, k + 1), F32), _inout(r.run_var0, kinds(i, k + 2), F32)
        self.all = (self.sc, self.sh, self.sm, self.si, self.rm, self.rv)

    def results(self):
        return [b.result()[0] for b in self.all]

    def args(self):
        return tuple(b.view for b in (self.rm, self.rv, self.sc, self.sh, self.sm, self.si))


@pytest.mark.parametrize('C', bx.C_EDGES)
def test_bn_stats_finalize_exact(C):
    """per-row-block partials on the bits (integers), save_mean on the bits at every M, the coefficients on the bits for M a power
    of two and within the derived ulp bounds elsewhere (bn_exact_util.forward_failures); channel 0 is constant: variance 0"""
    hip = _hip()
    n = bx.Counts()
    for i, (M, _) in enumerate(bx.cases(C)):
        q = bx.problem(M, C)
        momentum, zero = _forward_variant(i)
        has_gamma = i % 4 != 3                                  # gamma == NULL: fix_gamma, 1 everywhere
        r = bx.forward_ref(q, EPS, momentum, zero, has_gamma)
        what = 'sn_bn_stats + sn_bn_finalize M %d C %d momentum %g' % (M, C, momentum)
        x, ws = _in(q.x, kinds(i, 0)), _ws(M, C)
        g = _in(q.gamma, kinds(i, 1), F32) if has_gamma else None
        b = _in(q.beta, kinds(i, 2), F32)
        o = _FwdOut(i, C, r)
        hip.call('sn_bn_stats', x.view, M, C, x.pitch, ws.view, hip.stream())
        hip.call('sn_bn_finalize', ws.view, M, C, EPS, momentum, g.view if g else None, b.view, *(o.args() + (hip.stream(),)))
        blocks, _, rpb = bx.bn_grid(M, C)
        part = ws.result()[0, 2 * C:2 * C * (blocks + 1)].reshape(blocks, 2, C)
        starts = np.arange(0, M, rpb)
        _ok([bx.compare_exact(part[:, 0], np.add.reduceat(q.x, starts, axis=0), what + ' partial sums'),
             bx.compare_exact(part[:, 1], np.add.reduceat(q.x * q.x, starts, axis=0), what + ' partial sums of squares')])
        sc, sh, sm, si, rm, rv = o.results()
        _ok(bx.forward_failures(M, r, sc, sh, sm, si, rm, rv, what))
        assert r.var[0] == 0.0, what + ': the constant channel'
        _clean(what, ws, *o.all)
        n.add('cases')
        n.add('launches', 2)
        n.add('pow2' if bx.is_pow2(M) else 'other_M')
        n.add('exact_running' if r.run_exact else 'running_within_1_ulp')
    n['M'], n['seams'] = list(bx.m_edges(C)), sorted(bx.seams(C))
    n.log('bn_stats_finalize C %d' % C)
    assert n['cases'] == len(bx.cases(C)) >= 8 and n['pow2'] >= 2 and n['other_M'] >= 3 and n['exact_running'] >= 5


BLOCK_CASES = ((1, 64, 40), (31, 1000, 24), (32, 1024, 2056), (33, 100, 8), (512, 4096, 72), (513, 5000, 16), (1280, 8192, 96))


@pytest.mark.parametrize('nblk,M,C', BLOCK_CASES)
def test_bn_finalize_blocks_and_apply_blocks_exact(nblk, M, C):
    """sn_bn_finalize_blocks on integer partials made here (nblk row blocks; where nblk > M some are empty), against the same
    references; sn_bn_apply_blocks bit-equal to sn_bn_finalize_blocks + sn_bn_apply in every output"""
    hip = _hip()
    assert nblk in NBLKS
    i = NBLKS.index(nblk)
    q = bx.problem(M, C)
    momentum, zero = _forward_variant(i)
    r = bx.forward_ref(q, EPS, momentum, zero)
    part = np.stack([bx.block_partials(q.x, nblk), bx.block_partials(q.x * q.x, nblk)], axis=1).reshape(nblk, 2 * C)
    assert np.abs(part).max() < bx.FP32_EXACT
    pt = _in(part, 'dense', F32)
    x, g, b = _in(q.x, kinds(i, 0)), _in(q.gamma, kinds(i, 1), F32), _in(q.beta, kinds(i, 2), F32)
    n = bx.Counts()
    for act in bx.ACTS:
        what = 'sn_bn_finalize_blocks nblk %d M %d C %d act %d' % (nblk, M, C, act)
        o1, o2 = _FwdOut(i, C, r), _FwdOut(i, C, r, 1)
        y1, y2 = _out(M, C, kinds(i, act)), _out(M, C, kinds(i, act + 1))
        hip.call('sn_bn_finalize_blocks', pt.view, nblk, M, C, EPS, momentum, g.view, b.view, *(o1.args() + (hip.stream(),)))
        hip.call('sn_bn_apply', x.view, y1.view, M, C, x.pitch, y1.pitch, o1.sc.view, o1.sh.view, act, hip.stream())
        hip.call('sn_bn_apply_blocks', pt.view, nblk, x.view, y2.view, M, C, x.pitch, y2.pitch, EPS, momentum, g.view, b.view,
                 *(o2.args() + (act, hip.stream())))
        res1, res2 = o1.results(), o2.results()
        _ok(bx.forward_failures(M, r, *(res1 + [what])))
        for name, a1, a2 in zip(('scale', 'shift', 'save_mean', 'save_invstd', 'run_mean', 'run_var'), res1, res2):
            _ok([bx.compare_exact(a2, a1, what + ': sn_bn_apply_blocks against finalize + apply, ' + name)])
        got1 = y1.result()
        _ok([bx.compare_exact(y2.result(), got1, what + ': sn_bn_apply_blocks against finalize + apply, y')])
        # y against float64 with the kernel's own coefficients: one fma, one rounding to fp16
        pre = q.x * res1[0].astype(np.float64) + res1[1].astype(np.float64)
        want = (pre.astype(np.float32).astype(np.float64))
        want = want if act == 0 else np.maximum(want, 0.0) if act == 1 else np.clip(want, 0.0, 6.0)
        _ok([bx.compare_bound(got1, want, 0.5 * bx.ulp16(want) * (1 + 2.0 ** -10), what + ' y')])
        _clean(what, y1, y2, *(o1.all + o2.all))
        n.add('launches', 3)
    n.add('cases')
    n['M'], n['C'] = M, C
    n.log('bn_finalize_blocks nblk %d' % nblk)
    assert n['launches'] == 9


# -------------------------------------------------------------------------------------- sn_bn_backward, sn_bn_backward_blocks
def _dx_buffers(mode, q, i, k):
    """(accumulate, dx, the reference's acc) of an accumulate mode"""
    if mode == 'none':
        return None, _out(q.M, q.C, kinds(i, k)), None
    if mode == 'own':
        return _in(q.acc, kinds(i, k + 1)), _out(q.M, q.C, kinds(i, k)), q.acc
    dx = _inout(q.acc, kinds(i, k))
    return dx, dx, q.acc


@pytest.mark.parametrize('C', bx.C_EDGES)
def test_bn_backward_exact(C):
    """dbeta / dgamma on the bits onto a non-zero integer arena; dx on the bits for M a power of two and within
    bn_exact_util.dx_bound elsewhere, EVERY element compared, the edge elements included; accumulate none / own / aliased to dx;
    dx = NULL; sn_bn_backward_blocks on partials made here"""
    hip = _hip()
    n = bx.Counts()
    for i, (M, _) in enumerate(bx.cases(C)):
        q = bx.problem(M, C)
        small = M * C <= SMALL
        x, dy = _in(q.x, kinds(i, 0)), _in(q.dy, kinds(i, 1))
        sc, sh, iv = _in(q.scale, kinds(i, 2), F32), _in(q.shift, kinds(i, 3), F32), _in(q.invstd, kinds(i, 0), F32)
        ws = _ws(M, C)
        for act in bx.ACTS:
            r = bx.backward_ref(M, C, act)
            mu = _in(r.mean, kinds(i, 1 + act), F32)
            coefs = (sc.view, sh.view, mu.view, iv.view, act, ws.view)

            def launch(entry, mode, k, head=()):
                what = '%s act %d M %d C %d accumulate %s' % (entry, act, M, C, mode)
                acc, dx, ref_acc = _dx_buffers(mode, q, i, k) if mode != 'no dx' else (None, None, None)
                dg, db = _inout(q.dg0, kinds(i, k), F32), _inout(q.db0, kinds(i, k + 1), F32)
                hip.call(entry, *(head + (dy.view, x.view, acc.view if acc else None, dx.view if dx else None, M, C, dy.pitch, x.pitch,
                                          acc.pitch if acc else 0, dx.pitch if dx else 0) + coefs + (dg.view, db.view, hip.stream())))
                _ok(bx.backward_failures(q, r, dx.result() if dx else None, ref_acc, dg.result()[0], db.result()[0], what))
                _clean(what, dx, dg, db, ws)
                n.add('launches')
                n.add('accumulate_' + mode.replace(' ', '_'))

            modes = ACC_MODES if small else (ACC_MODES[(i + act) % 3],)
            for k, mode in enumerate(modes):
                launch('sn_bn_backward', mode, k)
            if small or act == bx.ACTS[i % 3]:
                launch('sn_bn_backward', 'no dx', 3)
                nblk = NBLKS[(i + act) % len(NBLKS)]
                part = np.stack([bx.block_partials(r.g, nblk), bx.block_partials(r.g * (q.x - r.mean), nblk)], axis=1).reshape(nblk, 2 * C)
                pt = _in(part, 'dense', F32)
                launch('sn_bn_backward_blocks', ACC_MODES[(i + act + 1) % 3], 2, (pt.view, nblk))
                n.add('blocks_nblk_%d' % nblk)
            n.add('edge_elements', r.edges.sum())
            n.add('elements', M * C)
        n.add('cases')
        n.add('pow2' if bx.is_pow2(M) else 'other_M')
    n['M'], n['seams'] = list(bx.m_edges(C)), sorted(bx.seams(C))
    n.log('bn_backward C %d' % C)
    assert n['cases'] == len(bx.cases(C)) >= 8 and n['pow2'] >= 2 and n['other_M'] >= 3
    assert min(n['accumulate_' + m] for m in ACC_MODES) >= n['cases'] and n['accumulate_no_dx'] >= n['cases']
    assert n['edge_elements'] >= 0.05 * 2 / 3 * n['elements']


# ------------------------------------------------------------------------------------------------------ sn_bn_frozen_backward
@pytest.mark.parametrize('C', bx.C_EDGES)
def test_bn_frozen_backward_exact(C):
    """eps = 0 and var in {0.25, 1, 4}: invstd is exact, so dx = scale * g [+ acc], dgamma and dbeta have ONE correct value; the
    dx-only and the parameter-only calls reproduce the combined one"""
    hip = _hip()
    n = bx.Counts()
    for i, (M, _) in enumerate(bx.cases(C)):
        q = bx.problem(M, C)
        x, dy = _in(q.x, kinds(i, 1)), _in(q.dy, kinds(i, 2))
        sc, sh = _in(q.scale, kinds(i, 3), F32), _in(q.shift, kinds(i, 0), F32)
        var = _in(1.0 / (q.invstd * q.invstd), kinds(i, 1), F32)
        ws = _ws(M, C)
        for act in _acts(i, M, C):
            r = bx.backward_ref(M, C, act)
            mu = _in(r.mean, kinds(i, 2 + act), F32)
            for k, mode in enumerate(ACC_MODES if M * C <= SMALL else (ACC_MODES[(i + act) % 3],)):
                what = 'sn_bn_frozen_backward act %d M %d C %d accumulate %s' % (act, M, C, mode)
                got = {}
                for call in ('combined', 'dx only', 'parameters only'):
                    acc, dx, ref_acc = _dx_buffers(mode, q, i, k) if call != 'parameters only' else (None, None, None)
                    par = call != 'dx only'
                    dg = _inout(q.dg0, kinds(i, k), F32) if par else None
                    db = _inout(q.db0, kinds(i, k + 1), F32) if par else None
                    hip.call('sn_bn_frozen_backward', dy.view, x.view, acc.view if acc else None, dx.view if dx else None, M, C, dy.pitch,
                             x.pitch, acc.pitch if acc else 0, dx.pitch if dx else 0, sc.view, sh.view, mu.view, var.view, 0.0, act,
                             ws.view if par else None, dg.view if par else None, db.view if par else None, hip.stream())
                    msgs = []
                    if dx:
                        got[call] = dx.result()
                        msgs.append(bx.compare_exact(got[call], r.dx_frozen + (0.0 if ref_acc is None else ref_acc), what + ' ' + call + ' dx'))
                    if par:
                        msgs += [bx.compare_exact(dg.result()[0], q.invstd * r.sgx + q.dg0, what + ' ' + call + ' dgamma'),
                                 bx.compare_exact(db.result()[0], r.sg + q.db0, what + ' ' + call + ' dbeta')]
                    _ok([m for m in msgs if m])
                    _clean(what + ' ' + call, dx, dg, db, ws)
                    n.add('launches')
                assert np.array_equal(got['combined'].view(np.int16), got['dx only'].view(np.int16)), what + ': dx only differs from combined'
                n.add('accumulate_' + mode)
            n.add('edge_elements', r.edges.sum())
        n.add('cases')
    n['M'], n['seams'] = list(bx.m_edges(C)), sorted(bx.seams(C))
    n.log('bn_frozen_backward C %d' % C)
    assert n['cases'] == len(bx.cases(C)) >= 8 and n['launches'] >= 3 * 3 * 3 * 6
    assert min(n['accumulate_' + m] for m in ACC_MODES) >= 3 * 6 and n['edge_elements'] > 0


# ------------------------------------------------------------------------------------------------------- the unfused siblings
SIBLING_SHAPES = ((1, 8), (3, 24), (85, 40), (257, 2056), (1000, 96), (4099, 256))


def _sibling_operands(rows, C, lo, hi):
    rs = np.random.RandomState(bx.case_seed((rows, C, lo, hi), 2))
    a, b = bx._ints(rs, (rows, C), -8, 8), bx._ints(rs, (rows, C), -8, 8)
    ref = bx._ints(rs, (rows, C), int(lo) - 3, int(hi) + 3)
    ref[0, :3] = (lo, hi, 0.0)
    return a, b, ref


def _with_acc(hip, n, entry, what, i, a, b_vals, ref, want, tail, clip):
    """relu / clip backward with accumulate none, own and aliased to y"""
    rows, C = a.shape
    av, rf = _in(a, kinds(i, 0)), _in(ref, kinds(i, 1))
    for k, mode in enumerate(ACC_MODES):
        if mode == 'none':
            acc, y, w = None, _out(rows, C, kinds(i, 2)), want
        elif mode == 'own':
            acc, y, w = _in(b_vals, kinds(i, 3)), _out(rows, C, kinds(i, 2)), want + b_vals
        else:
            y = _inout(b_vals, kinds(i, 3))
            acc, w = y, want + b_vals
        ap, pa = (acc.view if acc else None), (acc.pitch if acc else 0)
        if clip:
            hip.call(entry, av.view, rf.view, ap, y.view, rows, C, av.pitch, rf.pitch, pa, y.pitch, *(tail + (hip.stream(),)))
        else:
            hip.call(entry, av.view, ap, rf.view, y.view, rows, C, av.pitch, pa, rf.pitch, y.pitch, *(tail + (hip.stream(),)))
        _ok([bx.compare_exact(y.result(), w + 0.0, '%s accumulate %s' % (what, mode))])
        _clean(what, y)
        n.add('launches')
        n.add('accumulate_' + mode)


def test_ew_and_clip_exact():
    """sn_ew_f16 modes 0 / 1 / 2 (mask: ref > 0) and sn_clip_f16 forward / backward (mask: lo <= ref <= hi) with (0, 6) and an
    asymmetric range: on the bits, at least 5 % of `ref` exactly on an edge, accumulate none / own / aliased to the output, the
    forward forms in place too"""
    hip = _hip()
    n = bx.Counts()
    shapes = SIBLING_SHAPES + (GRID_STRIDE,)
    for i, (rows, C) in enumerate(shapes):
        big = (rows, C) == GRID_STRIDE
        for lo, hi in ((0.0, 6.0), (-2.0, 3.0)):
            if big:
                a = b = ref = _grid_stride_operands(int(lo) - 3, int(hi) + 3)
            else:
                a, b, ref = _sibling_operands(rows, C, lo, hi)
            edge = (ref == lo) | (ref == hi)
            assert edge.mean() >= 0.05 and (ref == 0).mean() >= 0.05
            n.add('edge_elements', edge.sum() + (ref == 0).sum())
            what = 'rows %d C %d range (%g, %g)' % (rows, C, lo, hi)
            # forward: out of place and in place
            for entry, want, args in (('sn_clip_f16', np.clip(a, lo, hi), (lo, hi, 0)), ('sn_ew_f16', np.maximum(a, 0.0), (0,))):
                for inplace in (False, True):
                    av = _inout(a, kinds(i, 0)) if inplace else _in(a, kinds(i, 0))
                    y = av if inplace else _out(rows, C, kinds(i, 1))
                    # (a, ref / b = NULL, accumulate / ref = NULL, y, ...: the two entry points agree up to the trailing arguments)
                    hip.call(entry, av.view, None, None, y.view, rows, C, av.pitch, 0, 0, y.pitch, *(args + (hip.stream(),)))
                    _ok([bx.compare_exact(y.result(), want + 0.0, '%s forward %s%s' % (entry, what, ' in place' if inplace else ''))])
                    _clean(entry + ' ' + what, y)
                    n.add('launches')
                    if big:
                        break
            if big:
                n.add('grid_stride')
                rf, y = _in(ref, 'dense'), _out(rows, C, '+8')
                hip.call('sn_clip_f16', rf.view, rf.view, None, y.view, rows, C, rf.pitch, rf.pitch, 0, y.pitch, lo, hi, 1, hip.stream())
                _ok([bx.compare_exact(y.result(), np.where((ref >= lo) & (ref <= hi), ref, 0.0), 'sn_clip_f16 backward grid-stride')])
                hip.call('sn_ew_f16', rf.view, None, rf.view, y.view, rows, C, rf.pitch, 0, rf.pitch, y.pitch, 2, hip.stream())
                _ok([bx.compare_exact(y.result(), np.where(ref > 0, ref, 0.0), 'sn_ew_f16 mode 2 grid-stride')])
                _clean('grid-stride', y)
                continue
            av, bv, y = _in(a, kinds(i, 0)), _in(b, kinds(i, 2)), _out(rows, C, kinds(i, 3))
            hip.call('sn_ew_f16', av.view, bv.view, None, y.view, rows, C, av.pitch, bv.pitch, 0, y.pitch, 1, hip.stream())
            _ok([bx.compare_exact(y.result(), a + b + 0.0, 'sn_ew_f16 add ' + what)])
            _clean('sn_ew_f16 add ' + what, y)
            n.add('launches')
            _with_acc(hip, n, 'sn_clip_f16', 'sn_clip_f16 backward ' + what, i, a, b, ref, np.where((ref >= lo) & (ref <= hi), a, 0.0), (lo, hi, 1), True)
            _with_acc(hip, n, 'sn_ew_f16', 'sn_ew_f16 mode 2 ' + what, i, a, b, ref, np.where(ref > 0, a, 0.0), (2,), False)
        n.add('cases')
    n.log('ew_and_clip')
    assert n['cases'] == len(shapes) and n['grid_stride'] == 2 and n['launches'] >= 2 * 6 * 11
    assert min(n['accumulate_' + m] for m in ACC_MODES) == 2 * 2 * len(SIBLING_SHAPES)
