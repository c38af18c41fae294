"""Exact-arithmetic oracle of the BatchNorm family ("Exact BatchNorm tests").

The integer-operand method of conv_exact_util.py carried over to the row-walking kernels of csrc/nn_ops.hip.  Operands: integer x
in [-4, 4], dy in [-3, 3], acc in [-8, 8]; per-channel scale and invstd from {0.5, 1, 2}; integer shift and mean in [-2, 2].  Then
  * every per-channel sum (sum x, sum x^2, sum g, sum g * (x - mean)) is an integer below 2^24: the fp32 partials, their block
    reduction and the double sum of the partials are exact in any order, so dbeta / dgamma / save_mean have ONE correct value;
  * the pre-activation x * scale + shift is a multiple of 0.5 of magnitude <= 10: 9-14 % of the elements sit EXACTLY on an
    activation edge (0, or 6), and the mask rule (relu: y > 0; relu6: 0 <= y <= 6) decides them -- no element is left out of a
    comparison;
  * for M a power of two every fp32 intermediate of bn_dx_coefs / bn_dx_value is exactly representable (asserted on the
    reference, `dx_chain_exact`), so the stored fp16 dx is a single rounding of the float64 value: bit for bit.  For any other M
    the fp32 chain rounds, and dx carries the derived bound of `dx_bound`.

This module holds what test_bn_exact_cases_cpu.py and test_gpu_bn_exact.py share: the restated launch arithmetic (`bn_grid`), the
case generator over its seams, operands and cached float64 references, the conditions, the comparisons and the perturbed
references that show the comparisons catch what they are for.  No device work happens at import time.

Out of scope: the dx kernels' own cap of 8192 row blocks (bn_grid(M, C, 8192)) is first met at M > 65 536 rows with C >= 2048; no
layer of a training step reaches it, and no case here does."""
import functools
import json
import os

import numpy as np

from conv_exact_util import FP16_EXACT, FP32_EXACT, PITCHES, Guarded, case_seed, first_mismatch, pitch_of  # noqa: F401

# ---- the launch arithmetic of csrc/nn_ops.hip, restated
BN_THREADS, BN_UNROLL, DX_CAP = 256, 4, 8192
C_EDGES = (8, 16, 24, 40, 72, 96, 256, 1024, 2048, 2056, 2560)
CAP_CS = (256, 1024, 2048)
ACTS = (0, 1, 2)
MIN_EDGE_SHARE = 0.05
U32 = 2.0 ** -24                 # unit roundoff of fp32, round to nearest


def div_up(a, b):
    return (a + b - 1) // b


def bn_rpp(C):
    """row lanes of a block: 256 threads over min(C / 8, 256) chunks (85 / 51 / 28 / 21 for C = 24 / 40 / 72 / 96: idle lanes)"""
    return BN_THREADS // min(C // 8, BN_THREADS)


def bn_reduce_cap(C):
    return min(512, max(256, (1 << 22) // (8 * C)))


def bn_grid(M, C, cap=None):
    """(row blocks, slabs, rows per block) of the row-walking kernels; cap: the reduction kernels' (default) or DX_CAP"""
    cap = bn_reduce_cap(C) if cap is None else cap
    rpp = bn_rpp(C)
    blocks = min(div_up(M, rpp * BN_UNROLL * 2), cap)
    rpb = div_up(div_up(M, blocks), rpp) * rpp
    return div_up(M, rpb), div_up(C // 8, BN_THREADS), rpb


def workspace_bytes(M, C):
    """sn_bn_workspace_bytes: fin (2C floats) + one [2][C] partial per row block, rounded up to 256 bytes"""
    return div_up(4 * 2 * C * (bn_grid(M, C)[0] + 1), 256) * 256


def last_rows(M, C, cap=None):
    blocks, _, rpb = bn_grid(M, C, cap)
    return M - (blocks - 1) * rpb


@functools.lru_cache(maxsize=None)
def seams(C):
    """name -> M of every seam a channel count must meet (ISSUE / DESIGN.md section 18)"""
    rpp = bn_rpp(C)
    s = {'one row': 1, 'three rows': 3, 'rpp - 1': rpp - 1, 'rpp': rpp, 'rpp + 1': rpp + 1,
         'unrolled loop once, no remainder': BN_UNROLL * rpp,
         'largest single block': 2 * BN_UNROLL * rpp, 'first two blocks': 2 * BN_UNROLL * rpp + 1,
         'power of two': 1024}
    fixed = {256: 2049, 1024: 257}          # (the examples of the issue; elsewhere the smallest such M)
    M = fixed.get(C, 2 * BN_UNROLL * rpp + 1)
    while not (bn_grid(M, C)[0] > 1 and last_rows(M, C) == 1):
        M += 1
    s['last block of one row'] = M
    if C in CAP_CS:
        s['first M beyond the reduce cap'] = bn_reduce_cap(C) * 2 * BN_UNROLL * rpp + 1
    if C == 256:
        s['beyond the reduce cap, 72 rows per block'] = 33000
    return {k: v for k, v in s.items() if v >= 1}


def m_edges(C):
    return tuple(sorted(set(seams(C).values())))


@functools.lru_cache(maxsize=None)
def cases(C=None):
    """(M, C) in a fixed order; of one channel count, or all"""
    if C is not None:
        return tuple((M, C) for M in m_edges(C))
    return tuple(mc for c in C_EDGES for mc in cases(c))


def is_pow2(M):
    return M & (M - 1) == 0


def kinds(i, k):
    """pitch kind of operand k of case i (conv_exact_util's rotation)"""
    return PITCHES[(i + k) % len(PITCHES)]


# ---- ulps
def _ulp(v, emin, bits):
    a = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(a)                                            # |v| = m * 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1
    return np.ldexp(1.0, np.where(a == 0, emin, np.maximum(e - 1, emin)) - bits)


def ulp16(v):
    """spacing of fp16 at |v| (2^-24 throughout the subnormal range)"""
    return _ulp(v, -14, 10)


def ulp32(v):
    return _ulp(v, -126, 23)


def fits(a, dtype):
    a = np.asarray(a, np.float64)
    return bool(np.all(a.astype(dtype).astype(np.float64) == a))


# ---- operands
class Ref(object):
    """plain attribute bag of read-only numpy arrays"""

    def freeze(self):
        for v in vars(self).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return self


def _ints(rs, shape, lo, hi, dtype=np.float64):
    return rs.randint(lo, hi + 1, size=shape).astype(dtype)


def _pre(q):
    return q.x * q.scale + q.shift


def edge_mask(pre, act):
    """the elements whose mask the activation's rule decides ON the edge"""
    if act == 1:
        return pre == 0.0
    if act == 2:
        return (pre == 0.0) | (pre == 6.0)
    return np.zeros(pre.shape, bool)


def act_pass(pre, act):
    """bn_act_pass: relu passes y > 0, relu6 passes 0 <= y <= 6 (mx.sym.clip's rule)"""
    if act == 0:
        return np.ones(pre.shape, bool)
    return pre > 0.0 if act == 1 else (pre >= 0.0) & (pre <= 6.0)


def _draw(M, C, salt):
    rs = np.random.RandomState(case_seed((M, C), salt))
    q = Ref()
    q.M, q.C, q.salt = M, C, salt
    q.x = _ints(rs, (M, C), -4, 4)
    q.dy = _ints(rs, (M, C), -3, 3)
    q.acc = _ints(rs, (M, C), -8, 8)
    q.scale = rs.choice([0.5, 1.0, 2.0], size=C)
    q.invstd = rs.choice([0.5, 1.0, 2.0], size=C)
    q.shift = _ints(rs, (C,), -2, 2)
    q.absmean = _ints(rs, (C,), 0, 2)
    rows = np.arange(M)
    # channel 0: constant (variance 0).  Channels 1 and C - 2: three rows of four sit exactly on y == 0; 2 and C - 1: on y == 6
    q.x[:, 0] = 3.0
    for c in (1, C - 2):
        q.x[:, c] = np.where(rows % 4 != 3, 2.0, q.x[:, c])
        q.scale[c], q.shift[c] = 1.0, -2.0
    for c in (2, C - 1):
        q.x[:, c] = np.where(rows % 4 != 2, 4.0, q.x[:, c])
        q.scale[c], q.shift[c] = 2.0, -2.0
    # the forward pass's parameters and state (gamma a signed power of two: scale = gamma * invstd is then ONE rounding)
    q.gamma = rs.choice([0.5, 1.0, 2.0, -1.0, -2.0], size=C)
    q.beta = _ints(rs, (C,), -4, 4)
    sign = rs.choice([-1.0, 1.0], size=C)
    q.run_mean0 = sign * _ints(rs, (C,), 8, 16)              # |run * momentum| > |stat * (1 - momentum)|: see forward_failures
    q.run_var0 = _ints(rs, (C,), 8, 16)
    q.dg0 = _ints(rs, (C,), -8, 8)                            # the gradient arena on entry (+= semantics)
    q.db0 = _ints(rs, (C,), -8, 8)
    return q


def edge_share(q, act):
    return float(edge_mask(_pre(q), act).mean())


@functools.lru_cache(maxsize=2)
def problem(M, C):
    """operands of one case.  A draw with too few edge elements (few rows of few channels) is drawn again under the next salt."""
    for salt in range(64):
        q = _draw(M, C, salt)
        if min(edge_share(q, 1), edge_share(q, 2)) >= MIN_EDGE_SHARE:
            break
    return q.freeze()


def block_partials(rows, nblk):
    """(M, C) -> (nblk, C): exact sums over nblk consecutive row ranges (empty ones where nblk > M: zero partials are valid)"""
    M = rows.shape[0]
    cs = np.concatenate([np.zeros((1, rows.shape[1])), np.cumsum(rows, axis=0)])
    b = (np.arange(nblk + 1) * M) // nblk
    return cs[b[1:]] - cs[b[:-1]]


# ---- backward references
DX_ROUNDINGS = 7


def dx_bound(r, acc=None, idx=None):
    """|got - want| <= ulp_fp16(want) / 2 + k * 2^-24 * (|scale * g| + |kb * x| + |kd| + |acc|), k = DX_ROUNDINGS = 7, counted in
    bn_dx_coefs + bn_dx_value (u = 2^-24 relative per rounding; scale and invstd are powers of two, dgamma = invstd * integer and
    dbeta are exact, so products with them do not round):
      invM = fl(1 / M)                                    1
      t    = fl(fl(invstd * dgamma) * invM)               inner product exact, outer 1            -> t carries 2
      kb   = -fl(scale * t)                               exact                                   -> kb carries 2
      kd   = fl(scale * fma(mean, t, -fl(dbeta * invM)))  dbeta / M carries 2 (invM, product), mean * t carries 2, the fma rounds
             once; the generator picks the sign of `mean` so that mean * t and -dbeta / M never cancel (|kd / scale| is the SUM of
             their magnitudes), so that rounding is relative to |kd|                              -> kd carries 3
      bn_dx_value: fma(kb, x, kd) rounds once on |kb x| + |kd|, fma(scale, g, .) once more, fadd(., acc) once more:
             scale * g carries 2, kb * x 2 + 3 = 5, kd 3 + 3 = 6, acc 1.
    The largest count is 6; one more covers the second-order terms ((1 + u)^6 - 1 - 6 u).  Then ONE rounding to fp16: half an ulp of
    the stored value, which is half an ulp of `want` (a value that crosses a binade rounds to the binade's edge)."""
    if idx is None:
        idx = (slice(None), slice(None))
    c = idx[1]
    a = 0.0 if acc is None else acc[idx]
    want = r.dx[idx] + a
    mag = np.abs(r.scale[c] * r.g[idx]) + np.abs(r.kb[c] * r.x[idx]) + np.abs(r.kd[c]) + np.abs(a)
    return 0.5 * ulp16(want) + DX_ROUNDINGS * U32 * mag


def _backward(q, act, row_weight=None, mean=None, flip=None):
    """float64 references of sn_bn_backward under activation `act`.  The perturbations: row_weight, the weight of every row in the
    SUMS (else one); flip, an (m, c) whose mask takes the other value; mean, the unperturbed reference's (else chosen here)"""
    r = Ref()
    r.M, r.C, r.act, r.x, r.scale = q.M, q.C, act, q.x, q.scale
    pre = _pre(q)
    r.edges = edge_mask(pre, act)
    r.g = q.dy * act_pass(pre, act) + 0.0
    if flip is not None:
        r.g[flip] = 0.0 if r.g[flip] else q.dy[flip]
    w = r.g if row_weight is None else r.g * row_weight[:, None]
    r.sg, sgx0 = w.sum(axis=0), (w * q.x).sum(axis=0)
    # the sign of mean: mean * t and -dbeta / M of one sign (dx_bound), t ~ sgx0 - mean * sg: mean * sgx0 * sg <= 0 does it
    r.mean = q.absmean * np.where(r.sg * sgx0 > 0, -1.0, 1.0) if mean is None else mean
    r.sgx = sgx0 - r.mean * r.sg                                  # sum g * (x - mean)
    r.dbeta, r.dgamma = r.sg + 0.0, q.invstd * r.sgx
    t = q.invstd * r.dgamma / q.M
    r.kb, r.kd = -q.scale * t, q.scale * (r.mean * t - r.dbeta / q.M)
    r.dx = q.scale * r.g + r.kb * q.x + r.kd + 0.0               # == scale * (g - dbeta / M - xhat * dgamma / M); + 0.0: no -0
    r.dx_frozen = q.scale * r.g + 0.0
    return r


@functools.lru_cache(maxsize=3)
def backward_ref(M, C, act):
    return _backward(problem(M, C), act).freeze()


def dx_chain_exact(q, r):
    """every fp32 intermediate of bn_dx_coefs / bn_dx_value, in the kernel's order, is exactly representable (float64 carries
    each of these dyadic values without rounding, so `fits` on the float64 value is the test): name of the first that is not"""
    invM = 1.0 / q.M
    t = q.invstd * r.dgamma * invM
    dbm = r.dbeta * invM
    f = r.mean * t - dbm
    inner = r.kb * q.x + r.kd
    s = q.scale * r.g + inner
    for name, v in (('invM', invM), ('dgamma', r.dgamma), ('t', t), ('kb', r.kb), ('dbeta * invM', dbm), ('fma(mean, t, .)', f),
                    ('kd', r.kd), ('fma(kb, x, kd)', inner), ('fma(scale, g, .)', s), ('dx', s + q.acc), ('dx, no acc', r.dx)):
        if not fits(v, np.float32):
            return name
    return None


def check_conditions(q):
    """what the zero tolerances rest on, asserted on the references alone"""
    M, C = q.M, q.C
    for name in ('x', 'dy', 'acc', 'shift', 'absmean', 'beta', 'run_mean0', 'run_var0', 'dg0', 'db0'):
        a = getattr(q, name)
        assert np.all(np.round(a) == a), ((M, C), name, 'not integral')
    for name in ('scale', 'invstd'):
        assert set(np.unique(getattr(q, name))) <= {0.5, 1.0, 2.0}, ((M, C), name)
    assert np.all(q.x[:, 0] == q.x[0, 0]), ((M, C), 'constant channel')
    pre = _pre(q)
    assert fits(pre, np.float16) and fits(np.clip(pre, 0, 6), np.float16), ((M, C), 'y')
    assert (q.x * q.x).sum(axis=0).max() < FP32_EXACT and np.abs(q.x).sum(axis=0).max() < FP32_EXACT, ((M, C), 'sum x^2')
    for c, edge in ((1, 0.0), (C - 2, 0.0), (2, 6.0), (C - 1, 6.0)):
        assert (pre[:, c] == edge).mean() >= 0.5, ((M, C), 'edge channel', c)
    for act in ACTS:
        r = backward_ref(M, C, act)
        if act:
            assert r.edges.mean() >= MIN_EDGE_SHARE, ((M, C), act, 'edge share', float(r.edges.mean()))
        assert np.abs(r.g).sum(axis=0).max() < FP32_EXACT, ((M, C), act, 'sum |g|')
        assert (np.abs(r.g) * (np.abs(q.x) + 2)).sum(axis=0).max() + 8 < FP32_EXACT, ((M, C), act, 'sum |g (x - mean)|')
        assert fits(r.dbeta + q.db0, np.float32) and fits(r.dgamma + q.dg0, np.float32), ((M, C), act, 'dbeta / dgamma')
        assert fits(r.dx_frozen + q.acc, np.float16), ((M, C), act, 'frozen dx')
        t = q.invstd * r.dgamma / M                                       # no cancellation in kd: what dx_bound's count rests on
        assert np.all(r.mean * t * (-r.dbeta / M) >= 0), ((M, C), act, 'kd cancels')
        if is_pow2(M):
            assert dx_chain_exact(q, r) is None, ((M, C), act, dx_chain_exact(q, r))
    return True


# ---- the comparisons (the GPU tests use exactly these)
def compare_exact(got, want, what):
    """'' or a message naming the first element whose bits differ"""
    bad = first_mismatch(got, want)
    if bad is None:
        return ''
    n = int((np.asarray(got, np.float64) != np.asarray(want, np.float64).astype(np.asarray(got).dtype).astype(np.float64)).sum())
    return '%s: %d of %d elements differ on the bits; first at %s: got %r want %r' % (
        what, n, np.asarray(want).size, bad, float(np.asarray(got)[bad]), float(np.asarray(want)[bad]))


def compare_bound(got, want, bound, what):
    """'' or a message naming the worst element with |got - want| > bound (NaN fails)"""
    err = np.abs(np.asarray(got, np.float64) - want)
    bad = ~(err <= bound)
    if not bad.any():
        return ''
    i = np.unravel_index(np.argmax(np.where(bad, err / np.maximum(bound, 1e-300), 0)), err.shape)
    return '%s: %d of %d elements beyond the bound; worst at %s: got %r want %r, |err| %.3g > %.3g' % (
        what, int(bad.sum()), err.size, tuple(int(j) for j in i), float(np.asarray(got)[i]), float(want[i]), float(err[i]),
        float(np.broadcast_to(bound, err.shape)[i]))


def compare_dx(got, r, acc, what):
    """dx of sn_bn_backward against the reference: on the bits for M a power of two, else within dx_bound; EVERY element.  (An
    element equal to fp16(want) is within half an fp16 ulp of want, inside the bound: the bound is evaluated at the others.)"""
    want = r.dx if acc is None else r.dx + acc
    if is_pow2(r.M):
        return compare_exact(got, want, what)
    got = np.asarray(got)
    idx = np.nonzero(~(got == want.astype(got.dtype)))
    if not len(idx[0]):
        return ''
    return compare_bound(got[idx], want[idx], dx_bound(r, acc, idx), what + ' (the %d elements that are not fp16(want))' % len(idx[0]))


def backward_failures(q, r, dx, acc, dgamma, dbeta, what):
    """all comparisons of one sn_bn_backward / _blocks launch; dx may be None (dx = NULL); the arena started at q.dg0 / q.db0"""
    out = [compare_exact(dbeta, r.dbeta + q.db0, what + ' dbeta'), compare_exact(dgamma, r.dgamma + q.dg0, what + ' dgamma')]
    if dx is not None:
        out.append(compare_dx(dx, r, acc, what + ' dx'))
    return [m for m in out if m]


# ---- forward references (sn_bn_stats + sn_bn_finalize, sn_bn_finalize_blocks)
FWD_ROUNDINGS = 2
SLACK = 1.0 + 2.0 ** -20          # second-order terms of a product of (1 + delta)s


def forward_ref(q, eps, momentum, zero_running, gamma=True):
    """float64 values and the fp32 restatement of bn_finalize_kernel + bn_fwd_coefs + bn_running.  Roundings of bn_fwd_coefs:
      invstd = (float)(1 / sqrt(var + eps))        1 (the double arithmetic below it is ~2^-29 of an fp32 ulp)
      scale  = fl(gamma * invstd)                  gamma is a signed power of two: exact                    -> 1 in all
      shift  = fma(-fl((float)mean * gamma), invstd, beta)   (float)mean 1, * gamma exact, invstd carries 1: FWD_ROUNDINGS = 2
               on |mean * scale|, then the fma's own half ulp of the result."""
    f32 = np.float32
    r = Ref()
    M = q.M
    g = q.gamma if gamma else np.ones(q.C)
    r.sum, r.sumsq = q.x.sum(axis=0), (q.x * q.x).sum(axis=0)
    r.mean = r.sum / M
    r.var = np.maximum(r.sumsq / M - r.mean * r.mean, 0.0)
    eps = float(f32(eps))
    r.invstd = 1.0 / np.sqrt(r.var + eps)
    r.scale = g * r.invstd
    r.shift = q.beta - r.mean * r.scale
    r.shift_bound = (0.5 * ulp32(r.shift) + FWD_ROUNDINGS * U32 * np.abs(r.mean * r.scale)) * SLACK
    # the restatement, rounding for rounding
    r.mean32, r.var32, r.invstd32 = r.mean.astype(f32), r.var.astype(f32), r.invstd.astype(f32)
    g32, b32 = g.astype(f32), q.beta.astype(f32)
    r.scale32 = g32 * r.invstd32
    p = (r.mean32 * g32).astype(np.float64)                        # (fl((float)mean * gamma): exact for gamma a power of two)
    r.shift32 = (q.beta - p * r.invstd32.astype(np.float64)).astype(f32)      # ONE rounding: the product is exact in float64
    # moving averages: run' = fma(run, m, fl(stat * (1 - m))), stat = (float)mean, (float)var (biased)
    m32 = f32(momentum)
    m, om = float(m32), float(f32(1.0) - m32)
    r.run_mean0 = np.zeros(q.C) if zero_running else q.run_mean0
    r.run_var0 = np.zeros(q.C) if zero_running else q.run_var0
    r.run_exact = bool(zero_running or momentum == 0.5)
    if r.run_exact:      # one rounding of the update of the stored statistic: the float64 expression is exact, the cast rounds once
        r.run_mean = r.run_mean0 * m + r.mean32.astype(np.float64) * om
        r.run_var = r.run_var0 * m + r.var32.astype(np.float64) * om
    else:                # the float64 value; two more roundings ((float)stat, fl(stat * (1 - m))) besides the result's: running_ok
        r.run_mean = r.run_mean0 * m + r.mean * om
        r.run_var = r.run_var0 * m + r.var * om
    return r.freeze()


def forward_failures(M, r, scale, shift, save_mean, save_invstd, run_mean, run_var, what):
    """save_mean on the bits for every M; invstd / scale / shift on the bits (of the restatement) for M a power of two, else within
    1 fp32 ulp of the float64 value (shift: r.shift_bound); running statistics on the bits where the update is exact, else
    within 1 ulp: |run0 * m| >= 7.2 > 2 > |stat * (1 - m)| puts the statistic's two roundings (each <= half an ulp of a value at
    least four times smaller than the result) under half an ulp of the result, whose own rounding is the other half."""
    out = [compare_exact(save_mean, r.mean, what + ' save_mean')]
    if is_pow2(M):
        out += [compare_exact(save_invstd, r.invstd32, what + ' save_invstd'), compare_exact(scale, r.scale32, what + ' scale'),
                compare_exact(shift, r.shift32, what + ' shift')]
    else:
        out += [compare_bound(save_invstd, r.invstd, ulp32(r.invstd), what + ' save_invstd'),
                compare_bound(scale, r.scale, ulp32(r.scale), what + ' scale'),
                compare_bound(shift, r.shift, r.shift_bound, what + ' shift')]
    if run_mean is not None:
        if r.run_exact:
            out += [compare_exact(run_mean, r.run_mean, what + ' run_mean'), compare_exact(run_var, r.run_var, what + ' run_var')]
        else:
            out += [compare_bound(run_mean, r.run_mean, ulp32(r.run_mean), what + ' run_mean'),
                    compare_bound(run_var, r.run_var, ulp32(r.run_var), what + ' run_var')]
    return [m for m in out if m]


def apply_ref(q, act):
    pre = _pre(q)
    return (pre if act == 0 else np.maximum(pre, 0.0) if act == 1 else np.clip(pre, 0.0, 6.0)) + 0.0


# ---- perturbed references: what a subtly wrong kernel would store (test_bn_exact_cases_cpu.py shows each one is caught)
PERTURBATIONS = ('row dropped', 'row doubled at a block seam', 'last chunk of the last slab zeroed', 'edge mask flipped',
                 'acc read after the store')


def _as_stored(r, q, dx):
    f32 = np.float32
    return dx.astype(np.float16), (r.dgamma + q.dg0).astype(f32), (r.dbeta + q.db0).astype(f32)


def stored(q, r, acc):
    """the reference as a correct kernel stores it: (dx fp16, dgamma fp32, dbeta fp32)"""
    return _as_stored(r, q, r.dx if acc is None else r.dx + acc)


def perturbed(q, act, kind):
    """(dx fp16, dgamma fp32, dbeta fp32, acc) of a kernel with ONE defect, accumulate = q.acc:
      row dropped / doubled       one row (with a non-zero g) of the first / at the seam of the second row block missing from /
                                  twice in the sums; every dx follows from the wrong dbeta / dgamma
      last chunk zeroed           the last 8 channels of dx (slab 2 where C > 2048) never written
      edge mask flipped           one element with y exactly on 0 (or 6) and dy != 0 takes the other side of bn_act_pass
      acc read after the store    dx = fp16(v) + fp16(v) of the aliased accumulate == dx launch"""
    r = backward_ref(q.M, q.C, act)
    M, C = q.M, q.C
    if kind in PERTURBATIONS[:2]:
        rpb = bn_grid(M, C)[2]
        start = 0 if kind == PERTURBATIONS[0] or rpb >= M else rpb
        row = start + int(np.argmax(np.abs(r.g[start:]).sum(axis=1) > 0))
        weight = np.ones(M)
        weight[row] = 0.0 if kind == PERTURBATIONS[0] else 2.0
        r2 = _backward(q, act, row_weight=weight, mean=r.mean)
        return _as_stored(r2, q, r2.dx + q.acc) + (q.acc,)
    if kind == PERTURBATIONS[2]:
        dx = r.dx + q.acc
        dx[:, C - 8:] = 0.0
        return _as_stored(r, q, dx) + (q.acc,)
    if kind == PERTURBATIONS[3]:
        hit = np.argwhere(r.edges & (q.dy != 0))
        assert len(hit), ((M, C), act, 'no edge element with a gradient')
        r2 = _backward(q, act, mean=r.mean, flip=tuple(hit[len(hit) // 2]))
        return _as_stored(r2, q, r2.dx + q.acc) + (q.acc,)
    if kind == PERTURBATIONS[4]:
        v = r.dx.astype(np.float16).astype(np.float64)
        return _as_stored(r, q, r.dx + v) + (q.acc,)
    raise ValueError(kind)


# ---- counts
class Counts(dict):
    def add(self, key, n=1):
        self[key] = self.get(key, 0) + int(n)

    def log(self, test):
        """one JSON line per test -- cases, launches, edge elements compared -- appended to the file that SNIPER_TEST_COUNTS names
        (unset: nothing is written)"""
        path = os.environ.get('SNIPER_TEST_COUNTS')
        if not path:
            return
        try:
            with open(path, 'a') as fh:
                fh.write(json.dumps(dict(self, test=test)) + '\n')
        except OSError:
            pass
