"""-m gpu: gradient accumulation -- sn_grad_accumulate bit for bit against its numpy restatement (tests/accumulate_ref.py) at every
edge of the peel / body / tail split and of the grid-stride loop, at every pair of pointer offsets, with canaries around both
ranges; its refusals; then windows of micro-steps on the small graph of tests/test_gpu_grad_guard.py, eager and captured: the window
is the sum, k = 1 is today's step, a partial window can be flushed, the guard, the clipping and the dynamic loss scale judge the
window once, and a Module and the R101 Trainer update once per k batches."""
import ctypes

import numpy as np
import pytest
import torch

import accumulate_ref as ref
import grad_guard_ref as gref
from gpu_util import dev
from test_gpu_grad_guard import ATOL, RTOL, SGD, SHAPES, _executor, _fixed, _gstate, _params, _same, mode, problem  # noqa: F401
from test_gpu_loss_scale import _aux, _differ, _lstate, _overflowing  # noqa: E402
from test_gpu_loss_scale import _executor as _scaled_executor  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = np.float32(-7.5)
PAD = 8


def _hip():
    from sniper_amd import hip
    return hip


def _limits():
    out = (ctypes.c_int32 * 3)()
    _hip().lib().call('sn_grad_accumulate_limits', out)
    return tuple(int(v) for v in out)


# ------------------------------------------------------------------------------------------------
# kernel
# ------------------------------------------------------------------------------------------------
# Every special value is written and examined as a bit pattern, never as a decimal or through a float comparison: a process in which
# the oracle has run flushes subnormals on the host (torch.set_flush_denormal), conversions and comparisons included.
P0, N0, INF, NINF, ONE, NAN, FLT_MAX, NFLT_MAX = 0, 0x80000000, 0x7f800000, 0xff800000, 0x3f800000, 0x7fc00000, 0x7f7fffff, 0xff7fffff
TINY, NTINY, MIN_NORMAL = 1, 0x80000001, 0x00800000            # the smallest subnormal, 2^-126
SPECIALS = [(N0, N0), (P0, N0), (N0, P0), (INF, NINF), (NINF, INF), (INF, ONE), (ONE, NINF), (NAN, ONE), (ONE, NAN), (INF, 0xffc00123),
            (FLT_MAX, FLT_MAX), (NFLT_MAX, NFLT_MAX), (FLT_MAX, NFLT_MAX), (TINY, TINY), (NTINY, TINY), (MIN_NORMAL, NTINY),
            (0x00200000, 0x00300000), (MIN_NORMAL, 0x80c00000), (ONE, 0x33800000), (ONE, 0x33c00000)]        # (acc, grad) bit patterns
# named by position: 0 + 0 of both signs, inf - inf, FLT_MAX + FLT_MAX, tiny + tiny, 2^-128 + 1.5 * 2^-128 (a subnormal sum),
# 2^-126 - 1.5 * 2^-126 (a normal pair with a subnormal sum), 1 + 2^-24 (a tie: to even), 1 + 1.5 * 2^-24 (rounds up)
I_NEG0, I_INF_INF, I_MAX_MAX, I_TINY_TINY, I_SUB_SUB, I_NORMAL_TO_SUB, I_TIE, I_UP = 0, 3, 10, 13, 16, 17, 18, 19


def _kinds(want):
    """which of the interesting results a float32 array holds, read from the bits"""
    b = ref.bits(want)
    e, m = (b >> 23) & 0xff, b & 0x7fffff
    return {name for name, hit in (('nan', (e == 255) & (m != 0)), ('inf', (e == 255) & (m == 0)), ('sub', (e == 0) & (m != 0)),
                                   ('-0', b == 0x80000000)) if hit.any()}


def _finite_bits(rs, n, near=None):
    """n floats uniform in sign, exponent (0 .. 254: subnormals to the largest binade) and mantissa; near: exponents within three of
    these floats' for every other element, so that half of the additions round instead of returning the larger operand"""
    exp = rs.randint(0, 255, n).astype(np.uint32)
    if near is not None:
        close = np.clip(((near.view(np.uint32) >> 23) & 0xff).astype(np.int64) + rs.randint(-3, 4, n), 0, 254).astype(np.uint32)
        exp = np.where(np.arange(n) % 2 == 0, close, exp)
    bits = (rs.randint(0, 2, n).astype(np.uint32) << 31) | (exp << 23) | rs.randint(0, 1 << 23, n).astype(np.uint32)
    return bits.view(np.float32)


def _contents(rs, n, turn):
    a = _finite_bits(rs, n)
    g = _finite_bits(rs, n, near=a)
    if n:
        where = rs.choice(n, size=min(n, len(SPECIALS)), replace=False)
        for j, p in enumerate(where):
            a.view(np.uint32)[p], g.view(np.uint32)[p] = SPECIALS[(j + turn) % len(SPECIALS)]
    return a, g


class _Pair(object):
    """acc and grad ranges of n floats at oa / og floats behind a 16-byte boundary, canaries before and after both"""

    def __init__(self, a, g, oa, og):
        n = a.size
        self.n, self.oa, self.og = n, oa, og
        self.host_a = np.full(oa + n + PAD, CANARY, np.float32)
        self.host_g = np.full(og + n + PAD, CANARY, np.float32)
        self.host_a[oa:oa + n], self.host_g[og:og + n] = a, g
        self.buf_a, self.buf_g = (torch.from_numpy(h.copy()).to(dev()) for h in (self.host_a, self.host_g))
        assert self.buf_a.data_ptr() % 16 == 0 and self.buf_g.data_ptr() % 16 == 0
        self.acc, self.grad = self.buf_a[oa:oa + n], self.buf_g[og:og + n]

    def run(self, first, max_blocks=0):
        hip = _hip()
        hip.call('sn_grad_accumulate', self.acc, self.grad, self.n, int(first), int(max_blocks), hip.stream())
        return self.buf_a.cpu().numpy(), self.buf_g.cpu().numpy()

    def check(self, got_a, got_g, first, what):
        n, oa = self.n, self.oa
        want = ref.accumulate(self.host_a[oa:oa + n], self.host_g[self.og:self.og + n], first)
        assert got_g.tobytes() == self.host_g.tobytes(), what                                     # the gradient and its canaries
        assert got_a[:oa].tobytes() == self.host_a[:oa].tobytes() and got_a[oa + n:].tobytes() == self.host_a[oa + n:].tobytes(), what
        if first:
            assert got_a[oa:oa + n].tobytes() == want.tobytes(), what                             # byte-equal, NaN payloads included
        else:
            assert ref.same_bits(got_a[oa:oa + n], want), (what, np.flatnonzero(got_a[oa:oa + n].view(np.uint32) != want.view(np.uint32))[:8])
        return want


def _edge_sizes():
    T, F, _ = _limits()
    S = T * F
    return [(n, 0) for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, S - 1, S, S + 1)] + [(n, 2) for n in (2 * S - 1, 2 * S, 2 * S + 1, 4 * S + 3)]


@pytest.mark.parametrize('oa', [0, 1, 2, 3])
def test_every_edge_at_every_pair_of_offsets(oa):
    """the accumulation arena at `oa` floats behind a 16-byte boundary, the gradient at every offset 0 .. 3, copy and add, sizes around
    the peel, the four-wide body, one block's span per trip and (max_blocks = 2) the grid-stride wrap"""
    T, F, cap = _limits()
    assert T % 64 == 0 and F % 4 == 0 and 256 <= cap <= 65535
    rs = np.random.RandomState(41 + oa)
    turn = 0
    hit = set()
    for og in range(4):
        for n, mb in _edge_sizes():
            for first in (1, 0):
                a, g = _contents(rs, n, turn)
                turn += 1
                pair = _Pair(a, g, oa, og)
                want = pair.check(*pair.run(first, mb), first=first, what=(n, mb, oa, og, first))
                if not first and n:
                    hit |= _kinds(want)
    assert hit == {'nan', 'inf', 'sub', '-0'}                  # the specials did what they are there for


def test_the_specials_one_by_one():
    """every special pair alone in the head, the body and the tail: 0 + -0, inf + -inf, FLT_MAX + FLT_MAX, subnormal sums ..."""
    a = ref.from_bits([p[0] for p in SPECIALS] * 3)
    g = ref.from_bits([p[1] for p in SPECIALS] * 3)
    want = ref.bits(ref.accumulate(a, g, False))
    assert want[I_NEG0] == 0x80000000 and want[1] == 0 and want[2] == 0                    # -0 + -0 = -0; 0 + -0 = +0
    assert want[I_INF_INF] & 0x7f800000 == 0x7f800000 and want[I_INF_INF] & 0x7fffff       # inf + -inf: NaN
    assert want[I_MAX_MAX] == 0x7f800000 and want[I_MAX_MAX + 1] == 0xff800000 and want[I_MAX_MAX + 2] == 0
    assert want[I_TINY_TINY] == 2 and want[I_TINY_TINY + 1] == 0 and want[I_TINY_TINY + 2] == 0x007fffff
    assert want[I_SUB_SUB] == 0x00500000 and want[I_NORMAL_TO_SUB] == 0x80400000          # subnormal sums, kept
    assert want[I_TIE] == 0x3f800000 and want[I_UP] == 0x3f800001
    for oa, og in ((0, 0), (3, 1), (1, 3)):
        for first in (1, 0):
            pair = _Pair(a, g, oa, og)
            pair.check(*pair.run(first), first=first, what=(oa, og, first))


@pytest.mark.parametrize('oa,og', [(1, 1), (0, 1)])
def test_a_larger_case_twice(oa, og):
    """n = 1300003 on the library's grid, one float off the 16-byte boundary (both arrays: the 16-byte path behind a peeled head;
    the gradient alone: the 4-byte loads): the same bits both times, numpy's bits"""
    n = 1300003
    rs = np.random.RandomState(8)
    a, g = _contents(rs, n, 0)
    outs = []
    for _ in range(2):
        pair = _Pair(a, g, oa, og)
        got_a, got_g = pair.run(0)
        pair.check(got_a, got_g, first=0, what=(oa, og))
        outs.append(got_a.tobytes())
    assert outs[0] == outs[1]
    pair = _Pair(a, g, oa, og)
    pair.check(*pair.run(1), first=1, what=(oa, og, 'copy'))


def test_refusals_leave_both_buffers_untouched():
    hip = _hip()
    rs = np.random.RandomState(3)
    a, g = _contents(rs, 64, 0)
    pair = _Pair(a, g, 0, 0)
    pa, pg = pair.acc.data_ptr(), pair.grad.data_ptr()
    one = torch.full((64,), 3.0, dtype=torch.float32, device=dev())
    before = one.clone()
    po = one.data_ptr()
    bad = [(None, pg, 4, 1, 0), (pa, None, 4, 0, 0), (None, None, 1, 1, 0), (pa, pg, -1, 1, 0), (pa + 2, pg, 4, 1, 0), (pa, pg + 1, 4, 0, 0),
           (pa, pg, 4, 1, -1), (pa, pg, 4, 0, 65536),
           (po, po, 8, 0, 0), (po, po + 16, 8, 1, 0), (po + 16, po, 8, 0, 0), (po, po + 28, 8, 1, 0), (po + 4, po, 60, 0, 0)]
    for args in bad:
        with pytest.raises(hip.SniperHipError) as e:
            hip.call('sn_grad_accumulate', *(args + (hip.stream(),)))
        assert 'sn_grad_accumulate' in str(e.value) and 'failed (1)' in str(e.value), args           # SN_ERR_ARG
    torch.cuda.synchronize()
    assert pair.buf_a.cpu().numpy().tobytes() == pair.host_a.tobytes() and pair.buf_g.cpu().numpy().tobytes() == pair.host_g.tobytes()
    assert torch.equal(one, before)
    # n = 0 succeeds (and launches nothing); ranges that touch without overlapping are taken
    assert hip.call('sn_grad_accumulate', pair.acc, pair.grad, 0, 1, 0, hip.stream()) == 0
    assert hip.call('sn_grad_accumulate', None, None, 0, 0, 0, hip.stream()) == 0
    assert pair.buf_a.cpu().numpy().tobytes() == pair.host_a.tobytes()
    assert hip.call('sn_grad_accumulate', po, po + 32, 8, 0, 0, hip.stream()) == 0
    assert torch.equal(one[:8], torch.full((8,), 6.0, device=dev())) and torch.equal(one[8:], before[8:])


# ------------------------------------------------------------------------------------------------
# step level: windows of micro-steps on the small graph, eager and captured
# ------------------------------------------------------------------------------------------------
def _arena(ex):
    return ex.arena_grad.cpu().numpy().copy()


def _sum(parts):
    s = parts[0]
    for p in parts[1:]:
        s = ref.accumulate(s, p, False)                   # float32, in arrival order, whatever mode the host's numpy is in
    assert s.dtype == np.float32 and s is not parts[0]
    return s


def _warm_up(ex, feed, n=2):
    """n windows of one micro-step at lr = 0 (nothing the optimizer owns moves: m = momentum * 0 - 0 * g, w += 0): afterwards a
    capturing executor captures at its next forward_backward and its next update"""
    before = _params(ex)
    for _ in range(n):
        ex.forward_backward(feed)
        if ex.accum is not None:
            ex.accumulate()
        ex.update(lr=0.0, wd=SGD['wd'], momentum=SGD['momentum'])
    assert _same(before, _params(ex)) == []


def test_the_window_is_the_sum(mode, problem):
    """1: k = 3, two windows over six feeds: the accumulation arena after the third accumulate() is (g1 + g2) + g3 in float32 of the
    three arenas read back, and the update is the plain update of a second executor on that sum -- nothing here assumes that a
    backward pass gives the same bits twice.  Between the windows' ends nothing moves; one update per window."""
    feeds = problem[2]
    a, plain = _executor(problem), _executor(problem)
    a.set_accumulate(3)
    _warm_up(a, feeds[0])
    assert _same(_params(a), _params(plain)) == []
    n0 = a.num_update
    graphs = []
    for w in range(2):
        before = _params(a)
        parts = []
        for j in range(3):
            a.forward_backward(feeds[3 * w + j])
            graphs.append(a._graph_fb)
            parts.append(_arena(a))
            assert a.accumulate() == j + 1
            assert _same(before, _params(a)) == [], (w, j)
        want = _sum(parts)
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        got = a.accum['arena'].cpu().numpy()
        assert got.tobytes() == want.tobytes(), (w, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert not np.array_equal(want, parts[2])
        plain.arena_grad.copy_(torch.from_numpy(want))
        for ex in (a, plain):
            ex.update(lr=SGD['lr'] * (w + 1), wd=SGD['wd'], momentum=SGD['momentum'])
        assert _same(_params(a), _params(plain)) == [], w
        moved = _same(before, _params(a))
        assert 'master' in moved and 'mom' in moved and 'w16' in moved and a.accum['pending'] == 0
    assert a.num_update - n0 == 2 and a.grad_arena() is a.accum['arena']
    if mode == 'captured':
        assert graphs[0] is not None and all(g is graphs[0] for g in graphs) and a._graph_up is not None
    else:
        assert graphs == [None] * 6 and a._graph_up is None


def test_k_1_is_todays_step(mode, problem):
    """2: set_accumulate(1) beside an untouched executor on copied gradients: bit-equal after each of four steps"""
    a, b = _executor(problem), _executor(problem)
    b.set_accumulate(1)
    assert b.accum is None and b.grad_arena() is b.arena_grad
    for i, feed in enumerate(problem[2][:4]):
        a.forward_backward(feed)
        b.arena_grad.copy_(a.arena_grad)
        for ex in (a, b):
            ex.update(lr=SGD['lr'] * (i + 1), wd=SGD['wd'], momentum=SGD['momentum'])
        assert _same(_params(a), _params(b)) == [], i
    assert (a._graph_up is not None) == (b._graph_up is not None) == (mode == 'captured')
    with pytest.raises(RuntimeError):
        b.accumulate()


def test_a_partial_window_is_flushed(mode, problem):
    """3: k = 3, two micro-steps, update: the plain update on g1 + g2; an update with nothing pending raises"""
    feeds = problem[2]
    a, plain = _executor(problem), _executor(problem)
    a.set_accumulate(3)
    with pytest.raises(RuntimeError):
        a.update(**SGD)
    assert a.num_update == 0
    parts = []
    for j in range(2):
        a.forward_backward(feeds[j])
        parts.append(_arena(a))
        assert a.accumulate() == j + 1
    want = _sum(parts)
    plain.arena_grad.copy_(torch.from_numpy(want))
    before = _params(a)
    a.update(**SGD)
    plain.update(**SGD)
    assert _same(_params(a), _params(plain)) == [] and 'master' in _same(before, _params(a))
    assert a.accum['pending'] == 0 and a.num_update == 1
    after = _params(a)
    with pytest.raises(RuntimeError):
        a.update(**SGD)
    assert _same(after, _params(a)) == [] and a.num_update == 1
    # the next window starts with a copy, not with what the flushed one left behind
    a.forward_backward(feeds[2])
    g = _arena(a)
    assert a.accumulate() == 1 and a.accum['arena'].cpu().numpy().tobytes() == g.tobytes()


def test_a_poisoned_micro_batch_skips_the_window(mode, problem):
    """4: the guard on, k = 3, inf written into one element of the gradient arena after the FIRST micro-step's forward_backward and
    before its accumulate: two clean micro-batches later the window's end changes nothing; the next window updates"""
    feeds = problem[2]
    ex = _executor(problem)
    ex.set_grad_guard(skip_nonfinite=True)
    ex.set_accumulate(3)
    _warm_up(ex, feeds[5])
    st0 = _gstate(ex)
    assert st0['steps'] == 2 and st0['skipped'] == 0
    before, n_up = _params(ex), ex.num_update
    for j in range(3):
        ex.forward_backward(feeds[j])
        if j == 0:
            ex.arena_grad[ex.arena_grad.numel() // 2 + 1] = float('inf')
        ex.accumulate()
    assert (ex._graph_fb is not None) == (mode == 'captured')
    ex.update(**SGD)
    assert _same(before, _params(ex)) == []
    st = _gstate(ex)
    assert st['steps'] == 3 and st['skipped'] == 1 and st['skip'] == 1 and st['nonfinite'] >= 1 and st['consecutive'] == 1
    assert ex.num_update == n_up + 1                       # the schedule counts windows
    for j in range(3):
        ex.forward_backward(feeds[3 + j])
        ex.accumulate()
    ex.update(**SGD)
    moved = _same(before, _params(ex))
    assert 'master' in moved and 'mom' in moved and 'w16' in moved
    st = _gstate(ex)
    assert st['steps'] == 4 and st['skipped'] == 1 and st['skip'] == 0 and st['consecutive'] == 0 and st['nonfinite'] == 0
    assert torch.isfinite(ex.arena_master).all() and torch.isfinite(ex.arena_mom).all()


def test_clipping_acts_on_the_sum(mode, problem):
    """5: clip_global_norm = half the norm of a window's sum: the plain update on 0.5 x the sum, at the bound of
    test_step_clipped_to_half_its_norm_is_the_plain_step_on_half_the_gradients (coef = 0.5 up to the 1e-6 of the rule's denominator)"""
    feeds = problem[2]
    a, b = _executor(problem), _executor(problem)
    b.set_accumulate(2)
    parts = []
    for j in range(2):
        b.forward_backward(feeds[j])
        parts.append(_arena(b))
        b.accumulate()
    s = _sum(parts)
    norm = gref.guard(s, 1.0, 0.0, False, np.zeros(8))[0]
    last = gref.guard(parts[1], 1.0, 0.0, False, np.zeros(8))[0]
    assert np.isfinite(norm) and norm > 1.0 and abs(norm - last) > 1e-3 * norm       # the sum's norm, not the last micro-batch's
    b.set_grad_guard(clip_global_norm=0.5 * norm)
    assert b.accum['pending'] == 2
    a.arena_grad.copy_(torch.from_numpy(s))
    a.arena_grad.mul_(0.5)
    a.update(**SGD)
    b.update(**SGD)
    st = _gstate(b)
    assert abs(st['coef'] - 0.5) < 1e-6 and st['coef'] != 1.0 and st['steps'] == 1
    assert abs(st['norm'] - norm) <= s.size * 2.0 ** -53 * norm
    pa, pb = _params(a), _params(b)
    print('max |momentum| %.3g' % float(pa['mom'].abs().max()))
    assert torch.allclose(pb['master'], pa['master'], rtol=RTOL, atol=ATOL) and torch.allclose(pb['mom'], pa['mom'], rtol=RTOL, atol=ATOL)
    assert torch.equal(b.arena_w16, b.arena_master.half())
    assert not torch.equal(pa['master'], _params(_executor(problem))['master'])


INIT = 2.0 ** 10
GS = 100.0 * 128.0 / INIT       # the graph's own loss scale: GS x 2^10 is the 100 x 128 the loss-scale tests run the same graph at


def test_dynamic_loss_scale_judges_the_window_once(mode, problem):
    """6a: k = 2, scale 2^10, restore_aux, the SECOND micro-batch's data holds an inf: the scale is halved once (2^9, scale_used 2^10),
    the parameters are unchanged and the moving statistics are those from before the window's FIRST micro-step -- not those from before
    its last micro-batch, which differ.  A clean window follows: the scale stays, clean = 1, the parameters move."""
    feeds = problem[2]
    ex = _scaled_executor(problem, GS)
    ex.set_loss_scale(INIT, restore_aux=True)
    ex.set_accumulate(2)
    assert ex.loss_scale['n_aux'] == 12
    before, aux_before = _params(ex), _aux(ex)
    ex.forward_backward(feeds[0])
    assert ex.accumulate() == 1
    aux_mid = _aux(ex)
    assert _differ(aux_before, aux_mid) != [] and all(torch.isfinite(t).all() for t in ex.aux.values())
    assert _lstate(ex)['scale'] == INIT
    ex.forward_backward(_overflowing(feeds[1]))
    assert ex.accumulate() == 2
    ex.update(**SGD)
    st = _lstate(ex)
    assert st['scale'] == INIT / 2 and st['scale_used'] == INIT and st['backoffs'] == 1 and st['clean'] == 0 and st['growths'] == 0
    g = _gstate(ex)
    assert g['skip'] == 1 and g['nonfinite'] > 0 and g['steps'] == 1 and g['skipped'] == 1
    assert _same(before, _params(ex)) == []
    assert _differ(aux_before, _aux(ex)) == []
    for j in range(2):
        ex.forward_backward(feeds[2 + j])
        ex.accumulate()
        assert _lstate(ex)['scale'] == INIT / 2          # one scale for the whole window
    ex.update(**SGD)
    st = _lstate(ex)
    assert st['scale'] == INIT / 2 and st['scale_used'] == INIT / 2 and st['clean'] == 1 and st['backoffs'] == 1
    g = _gstate(ex)
    assert g['skip'] == 0 and g['steps'] == 2 and g['skipped'] == 1 and g['consecutive'] == 0
    moved = _same(before, _params(ex))
    assert 'master' in moved and 'mom' in moved and 'w16' in moved
    assert all(torch.isfinite(t).all() for t in ex.aux.values()) and _differ(aux_before, _aux(ex)) != []
    assert torch.isfinite(ex.arena_master).all() and torch.isfinite(ex.arena_mom).all()
    assert (ex._graph_fb is not None) == (mode == 'captured')


def test_a_fixed_dynamic_scale_window_is_the_static_scale_window(mode, problem):
    """6b: what test_fixed_dynamic_scale_is_the_static_scale states for a step, for windows of two: a static graph with the scale
    in its grad_scale attributes, lr / S, wd * S, against the same graph with set_loss_scale(S, growth_interval=0) and the true lr /
    wd, both accumulating: the gradient arena bit-equal after every forward_backward, the accumulation arena bit-equal after every
    accumulate, the moving statistics bit-equal, and masters / momentum / fp16 and transposed copies bit-equal after each update: S
    is a power of two, so lr / S, wd * S and the 1 / S inside the guarded update's coefficient scale every product exactly"""
    feeds = problem[2]
    a, b = _scaled_executor(problem, GS * INIT), _scaled_executor(problem, GS)
    b.set_loss_scale(INIT, growth_interval=0)
    for ex in (a, b):
        ex.set_accumulate(2)
    for w in range(2):
        for j in range(2):
            for ex in (a, b):
                ex.forward_backward(feeds[2 * w + j])
            assert torch.equal(a.arena_grad.view(torch.int32), b.arena_grad.view(torch.int32)), (w, j)
            for ex in (a, b):
                ex.accumulate()
            assert torch.equal(a.accum['arena'].view(torch.int32), b.accum['arena'].view(torch.int32)), (w, j)
            assert _differ(_aux(a), _aux(b)) == [], (w, j)
        a.update(lr=SGD['lr'] / INIT, wd=SGD['wd'] * INIT, momentum=SGD['momentum'])
        b.update(**SGD)
        pa, pb = _params(a), _params(b)
        for key in ('master', 'mom'):
            print('window %d: %s max |a - b| %.3g, bit-equal %s' % (w, key, float((pa[key] - pb[key]).abs().max()), torch.equal(pa[key], pb[key])))
        assert _same(pa, pb) == [], w
    st = _lstate(b)
    assert st['scale'] == INIT and st['scale_used'] == INIT and st['clean'] == 2 and st['growths'] == 0 and st['backoffs'] == 0
    assert b.guard['state'].cpu()[4] == 2 and b.guard['state'].cpu()[5] == 0 and a.num_update == b.num_update == 2


class _CountingScheduler(object):
    base_lr = None

    def __init__(self):
        self.calls = []

    def __call__(self, num_update):
        self.calls.append(num_update)
        return 1e-4


def test_module_updates_once_per_window(problem):
    """7a: a Module with accumulate = 2 over four forward_backward + update calls: the parameters change after calls 2 and 4 only, the
    scheduler is called with 1 and 2"""
    import sniper_amd.mx as mx
    from test_gpu_engine import _mini_graph
    P, AUX, feeds = problem
    sym = _mini_graph(mx, 3)
    labels = ['label', 'bbox_target', 'bbox_weight']
    mod = mx.mod.Module(sym, data_names=['data'], label_names=labels, context=[mx.gpu(0)], fixed_param_names=_fixed(sym))
    mod.bind(data_shapes=[('data', SHAPES['data'])], label_shapes=[(k, SHAPES[k]) for k in labels], for_training=True)
    mod.init_params(arg_params=P, aux_params=AUX)
    sched = _CountingScheduler()
    mod.init_optimizer(optimizer='sgd', optimizer_params={'accumulate': 2, 'learning_rate': 1e-4, 'momentum': 0.9, 'wd': 1e-3,
                                                          'lr_scheduler': sched})
    assert mod.exe.accum is not None and mod.exe.accum['k'] == 2 and mod.accumulate_state() == {'k': 2, 'pending': 0, 'updates': 0}
    changed = []
    for call in range(1, 5):
        before = _params(mod.exe)
        mod.forward_backward(mx.io.DataBatch(data=[feeds[call]['data']], label=[feeds[call][k] for k in labels]))
        mod.update()
        if _same(before, _params(mod.exe)):
            changed.append(call)
        assert mod.accumulate_state()['pending'] == call % 2
    assert changed == [2, 4] and sched.calls == [1, 2]
    assert mod.accumulate_state() == {'k': 2, 'pending': 0, 'updates': 2} and mod.exe.num_update == 2


def test_trainer_with_accumulation():
    """7b: the R101 Trainer with accumulate = 2: four steps, two updates, everything finite"""
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=2, n_images=8, seed=0, accumulate=2)
    ex = tr.mod.exe
    assert ex.accum is not None and ex.accum['k'] == 2 and tr.mod.opt['accumulate'] == 2
    before = ex.arena_master.clone()
    for i in range(4):
        outs = tr.step()
        for o in outs:
            assert np.isfinite(o.asnumpy()).all()
        if i == 0:
            assert torch.equal(before, ex.arena_master)        # the first batch of a window updates nothing
    assert ex.num_update == 2 and tr.mod.accumulate_state() == {'k': 2, 'pending': 0, 'updates': 2}
    assert torch.isfinite(ex.arena_master).all() and torch.isfinite(ex.arena_mom).all() and not torch.equal(before, ex.arena_master)
