"""Exact-arithmetic oracle of the convolution family ("Exact convolution tests").

Small integer operands: every product and every partial sum of a convolution is an integer below 2^24, so fp32 accumulation is
exact in any order, on any tile, split or slab, every stored fp16 value is an integer of magnitude <= 2048 and therefore exact,
and the float64 reference is the ONLY correct answer: the tolerance is zero.  This module holds what the CPU test
(test_conv_exact_cases_cpu.py) and the GPU tests (test_gpu_conv_exact.py) share: the deterministic case generator over the tile
edges, the operands and cached float64 references, the conditions each case is built under, the bit comparison, and (GPU only)
the guarded device buffers.  No device work happens at import time."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as Fnn

# ---- the edges the generator covers (row tiles 64 / 128 / 160 / 256, column tiles 64 / 128 / 256, K-steps of 64 channels, ring
# depths 2 / 3 / 4; the weight gradient's 32-pixel units)
M_EDGES = (1, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 321)
# 42: the scalar epilogue (its data gradient contracts over 48); 65 / 130: the Cout % 4 != 0 epilogue of the pipelined kernel
COUT_EDGES = (8, 16, 42, 64, 65, 72, 128, 130, 136, 256, 264)
CIN_EDGES = (8, 24, 64, 72, 128, 136, 192, 200, 256, 320)
# (K, stride, pad, dil); the last: a whole output ring that sees only padding
GEOMS = ((1, 1, 0, 1), (1, 2, 0, 1), (3, 1, 1, 1), (3, 1, 0, 1), (3, 2, 1, 1), (3, 1, 2, 2), (5, 2, 2, 1), (3, 1, 2, 1))
MAX_PIXELS, MAX_CHANNELS = 400, 320

FP16_EXACT = 2048            # every integer of magnitude <= 2048 is an fp16 value
FP32_EXACT = 1 << 24         # ... below 2^24 an fp32 value
MAX_ZERO_SHARE = 0.10


def out_dim(H, K, s, p, d):
    return (H + 2 * p - d * (K - 1) - 1) // s + 1


def in_dim(Ho, K, s, p, d, even):
    """an input extent whose output extent is Ho (stride 2: the even or the odd one of the two), or 0 when there is none"""
    H = (Ho - 1) * s + d * (K - 1) + 1 - 2 * p
    if s == 2 and (H % 2 == 0) != even:
        H += 1
    return H if H >= 1 and out_dim(H, K, s, p, d) == Ho else 0


def factorisations(M):
    """(N, Ho, Wo) with N * Ho * Wo == M, in a fixed order"""
    out = []
    for N in range(1, M + 1):
        if M % N:
            continue
        for Ho in range(1, M // N + 1):
            if (M // N) % Ho == 0:
                out.append((N, Ho, M // N // Ho))
    return out


def feasible(M, geom):
    """geometry (3, 1, 2, 1) has Ho = H + 2 >= 3: an M with no two factors >= 3 (1 and the primes 127, 257) cannot take it"""
    K, s, p, d = geom
    return any(in_dim(Ho, K, s, p, d, False) and in_dim(Wo, K, s, p, d, False) for (_, Ho, Wo) in factorisations(M))


def _shape_for(M, geom, turn):
    """an admissible (N, H, W) of an M edge under a geometry, picked by `turn` (the case's position in the list): at most 8 images
    where M allows it, so that one image, several images (a row tile straddles their boundary) and every row length come up;
    stride 2 alternates even destination extents (the data gradient's parity-class walk) and odd ones (the every-tap walk)"""
    K, s, p, d = geom
    even = turn % 2 == 0
    cands = []
    for (N, Ho, Wo) in factorisations(M):
        H, W = in_dim(Ho, K, s, p, d, even), in_dim(Wo, K, s, p, d, even)
        if H and W and (N <= 8 or Ho * Wo == 1 or not cands):
            cands.append((N, H, W))
    return cands[zlib.crc32(repr((M, geom, turn)).encode()) % len(cands)]


# cases outside the covering loop: row lengths of 32 and 33 output pixels under K > 1 (the weight gradient's 32-pixel unit, whole
# and one over), an odd number of units, and -- below this line -- the smallest failing case of every bug the sweep has found,
# each with a comment naming the cause
FIXED_CASES = (
    (1, 3, 33, 64, 72, 3, 1, 1, 1),        # Wo = 33: 2 units per row, 3 rows
    (3, 1, 33, 24, 136, 3, 1, 1, 1),       # Wo = 33 across images, Ho = 1
    (1, 5, 34, 72, 64, 3, 1, 0, 1),        # Wo = 32, Ho = 3: 3 units
    (1, 6, 66, 8, 130, 3, 2, 1, 1),        # stride 2, Wo = 33, even destination extents
    (2, 2, 35, 128, 16, 3, 1, 2, 2),       # dilation 2, Wo = 35 > 32, M = 140
)


@functools.lru_cache(maxsize=None)
def cases():
    """The covering set: tuples (N, H, W, Cin, Cout, K, stride, pad, dil) in which every feasible (M, Cout), (M, geometry),
    (Cout, Cin) and (Cin, geometry) pair of the edge lists occurs.  Greedy and deterministic: each new case takes the next uncovered
    (M, Cout) pair -- or, when those are used up, the M and Cout that still have the most uncovered partners -- and the geometry
    and Cin that cover the most pairs still open."""
    open_mo = [(m, o) for m in M_EDGES for o in COUT_EDGES]
    open_mg = {(m, g) for m in M_EDGES for g in GEOMS if feasible(m, g)}
    open_oc = {(o, c) for o in COUT_EDGES for c in CIN_EDGES}
    open_cg = {(c, g) for c in CIN_EDGES for g in GEOMS}
    out = []
    while open_mo or open_mg or open_oc or open_cg:
        if open_mo:
            m, o = open_mo.pop(0)
        else:
            m = max(M_EDGES, key=lambda mm: sum((mm, g) in open_mg for g in GEOMS))
            o = max(COUT_EDGES, key=lambda oo: sum((oo, c) in open_oc for c in CIN_EDGES))
        g, c = max(((gg, cc) for gg in GEOMS if feasible(m, gg) for cc in CIN_EDGES),
                   key=lambda gc: ((m, gc[0]) in open_mg) + ((o, gc[1]) in open_oc) + ((gc[1], gc[0]) in open_cg))
        N, H, W = _shape_for(m, g, len(out))
        out.append((N, H, W, c, o) + g)
        open_mg.discard((m, g))
        open_oc.discard((o, c))
        open_cg.discard((c, g))
    return tuple(out) + FIXED_CASES


def infeasible_pairs():
    return tuple((m, g) for m in M_EDGES for g in GEOMS if not feasible(m, g))


def case_dims(case):
    N, H, W, C, O, K, s, p, d = case
    Ho, Wo = out_dim(H, K, s, p, d), out_dim(W, K, s, p, d)
    return Ho, Wo, N * Ho * Wo


def case_seed(case, salt=0):
    """from the tuple itself (hash() changes between processes)"""
    return zlib.crc32(repr((tuple(case), salt)).encode()) & 0x7FFFFFFF


# ---- operands
def int_operand(rs, shape, lo, hi):
    return rs.randint(lo, hi + 1, size=shape).astype(np.float64)


def masked_weights(rs, shape, contraction):
    """integers in [-2, 2], kept with probability min(1, 64 / contraction): the sums stay small however long the contraction"""
    w = int_operand(rs, shape, -2, 2)
    keep = rs.random_sample(shape) < min(1.0, 64.0 / contraction)
    return w * keep


def bn_coefficients(rs, C):
    """scale in {0.5, 1, 2}, integer mean, shift = integer + 0.5, such that no pre-activation scale * x + shift of an integer
    x in [-3, 3] sits on 0 or 6 (whose rule belongs to sn_bn_backward).  scale 1 and 2 give half-integers whatever the integer; a
    scale of 0.5 gives integers for odd x, in [j - 1, j + 2] for shift = j + 0.5, so j is drawn where that range misses 0 and 6."""
    scale = rs.choice([0.5, 1.0, 2.0], size=C)
    j = rs.randint(-3, 4, size=C).astype(np.float64)
    j = np.where(scale == 0.5, rs.choice([-4.0, 2.0, 3.0, 9.0], size=C), j)
    mean = rs.randint(-2, 3, size=C).astype(np.float64)
    return scale, j + 0.5, mean


class Problem(object):
    """operands and float64 references of one case (all numpy float64, NCHW / OIHW; read-only)"""


def _build(case, salt, grads=True):
    N, H, W, C, O, K, s, p, d = case
    rs = np.random.RandomState(case_seed(case, salt))
    q = Problem()
    q.case, q.salt = tuple(case), salt
    q.x = int_operand(rs, (N, C, H, W), -3, 3)
    q.w = masked_weights(rs, (O, C, K, K), C * K * K / 2.0 ** salt)
    xt = torch.from_numpy(q.x).requires_grad_(grads)
    wt = torch.from_numpy(q.w).requires_grad_(grads)
    y = Fnn.conv2d(xt, wt, None, s, p, d)
    q.dy = int_operand(rs, tuple(y.shape), -3, 3)
    if grads:
        y.backward(torch.from_numpy(q.dy))
        q.dx, q.dw = xt.grad.numpy() + 0.0, wt.grad.numpy() + 0.0
    else:               # (forward-only problems: the split-K shapes)
        q.dx, q.dw = np.zeros_like(q.x), np.zeros_like(q.w)
    q.y = y.detach().numpy() + 0.0
    q.bias = int_operand(rs, (O,), -8, 8)
    q.bias_q = rs.randint(-32, 33, size=(O,)) * 0.25                       # the quarter variant: fp32 output only
    q.res = int_operand(rs, q.y.shape, -8, 8)
    q.acc = int_operand(rs, q.x.shape, -8, 8)
    q.dw0 = int_operand(rs, q.w.shape, -8, 8)                               # dw on entry (+= semantics)
    q.pre = q.y + q.bias.reshape(1, O, 1, 1) + q.res                       # the pre-activation of bias + residual + ReLU
    q.y_brr = np.maximum(q.pre, 0.0)
    q.y_q = q.y + q.bias_q.reshape(1, O, 1, 1)
    q.dx_acc = q.dx + q.acc
    q.bn_scale, q.bn_shift, q.bn_mean = bn_coefficients(rs, C)
    q.bn_x = int_operand(rs, q.x.shape, -3, 3)
    for v in vars(q).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return q


def zero_share(q):
    return max(float((q.y == 0).mean()), float((q.pre == 0).mean()))


def check_conditions(q):
    """what the zero tolerance rests on, asserted on the reference alone"""
    def integral(a, unit=1.0):
        return bool(np.all(np.round(a / unit) * unit == a))
    for name in ('x', 'w', 'dy', 'bias', 'res', 'acc', 'dw0', 'bn_x', 'bn_mean', 'y', 'dx', 'dw', 'pre', 'y_brr', 'dx_acc'):
        assert integral(getattr(q, name)), (q.case, name, 'not integral')
    assert integral(q.bias_q, 0.25) and integral(q.y_q, 0.25), (q.case, 'quarter bias')
    for name in ('x', 'w', 'dy', 'res', 'acc', 'bn_x', 'y', 'y_brr', 'dx', 'dx_acc'):       # stored as fp16
        assert np.abs(getattr(q, name)).max() <= FP16_EXACT, (q.case, name, np.abs(getattr(q, name)).max())
    for name in ('dw', 'dw0', 'y_q', 'y', 'dx', 'pre'):                                      # fp32 values
        assert np.abs(getattr(q, name)).max() + np.abs(q.dw0).max() < FP32_EXACT, (q.case, name)
    assert 256 * np.abs(q.y).max() ** 2 < FP32_EXACT, (q.case, 'sum of squares of a row tile', np.abs(q.y).max())
    assert 256 * np.abs(q.dx).max() * (np.abs(q.bn_x).max() + np.abs(q.bn_mean).max()) < FP32_EXACT, (q.case, 'BatchNorm-backward sums')
    assert zero_share(q) <= MAX_ZERO_SHARE, (q.case, 'zero share', zero_share(q))


@functools.lru_cache(maxsize=None)
def problem(case, grads=True):
    """the case's operands and references, computed once however many configurations run it.  A draw whose outputs are zero too
    often (a short contraction; a small image under a large kernel, most of whose taps are padding) is drawn again under the next
    salt with twice the weight density: seed and density change, the caps do not."""
    for salt in range(16):
        q = _build(tuple(case), salt, grads)
        if zero_share(q) <= MAX_ZERO_SHARE:
            break
    check_conditions(q)
    return q


# ---- restatements in numpy float64 (NHWC row views)
def rows_nhwc(a_nchw):
    """(N, C, H, W) -> (N * H * W, C)"""
    a = np.asarray(a_nchw)
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1, a.shape[1])


def w_rows(w_oihw):
    """(O, I, KH, KW) -> [O][KH * KW * I], the library's weight layout"""
    O, I, KH, KW = w_oihw.shape
    return np.ascontiguousarray(w_oihw.transpose(0, 2, 3, 1)).reshape(O, KH * KW * I)


def wt_rows(w_oihw, O_pad):
    """-> [I][KH * KW * O_pad]: the data gradient's transposed copy, zero in the padding lanes"""
    O, I, KH, KW = w_oihw.shape
    out = np.zeros((I, KH * KW, O_pad))
    out[:, :, :O] = w_oihw.transpose(1, 2, 3, 0).reshape(I, KH * KW, O)
    return out.reshape(I, KH * KW * O_pad)


def bn_mask(bn_x_rows, scale, shift, act):
    pre = bn_x_rows * scale + shift
    assert not np.any(pre == 0.0) and not np.any(pre == 6.0)
    if act == 0:
        return np.ones_like(pre)
    return (pre > 0).astype(np.float64) if act == 1 else ((pre >= 0) & (pre <= 6)).astype(np.float64)


def block_sums(rows, bm):
    """(M, C) -> (ceil(M / bm), C): the sums over each row tile"""
    M = rows.shape[0]
    return np.stack([rows[i:i + bm].sum(axis=0) for i in range(0, M, bm)])


# ---- the comparison
def first_mismatch(got, want):
    """index of the first element whose BITS differ, or None.  `want` (float64) is cast to got's type."""
    got = np.asarray(got)
    want = np.asarray(want, np.float64).astype(got.dtype)
    assert got.shape == want.shape, (got.shape, want.shape)
    bits = {2: np.int16, 4: np.int32, 8: np.int64}[got.dtype.itemsize]
    bad = np.ascontiguousarray(got).view(bits) != np.ascontiguousarray(want).view(bits)
    if not bad.any():
        return None
    return tuple(int(i) for i in np.argwhere(bad)[0])


def exact_equal(got, want):
    return first_mismatch(got, want) is None


def assert_exact_rows(got_rows, want_rows, what, row_len=None, rows_img=None, tile=None):
    """(M, C) rows against the float64 reference, on the bits; the message names the first differing element as (n, y, x, c) and
    the (row, column) tile it falls in"""
    bad = first_mismatch(got_rows, want_rows)
    if bad is None:
        return
    m, c = bad
    where = 'row %d channel %d' % (m, c)
    if row_len and rows_img:
        where += ' (n, y, x, c) = (%d, %d, %d, %d)' % (m // rows_img, m % rows_img // row_len, m % row_len, c)
    if tile:
        where += ' tile (%d, %d) of %d x %d' % (m // tile[0], c // tile[1], tile[0], tile[1])
    n_bad = int((np.asarray(got_rows, np.float64) != np.asarray(want_rows, np.float64)).sum())
    raise AssertionError('%s: %d of %d elements differ; first %s: got %r want %r'
                         % (what, n_bad, np.asarray(want_rows).size, where, float(got_rows[bad]), float(np.asarray(want_rows)[bad])))


def perturbed_forward(q, pixel, tap, chunk, factor):
    """the forward reference with ONE (pixel, tap, 8-channel chunk) contribution scaled by `factor` (0: dropped, 2: doubled): what a
    kernel that skipped or repeated that chunk would store.  pixel = (n, oy, ox), tap = (kh, kw)."""
    N, H, W, C, O, K, s, p, d = q.case
    n, oy, ox = pixel
    kh, kw = tap
    sy, sx = oy * s - p + kh * d, ox * s - p + kw * d
    y = q.y.copy()
    if 0 <= sy < H and 0 <= sx < W:
        c0 = chunk * 8
        y[n, :, oy, ox] += (factor - 1.0) * (q.w[:, c0:c0 + 8, kh, kw] @ q.x[n, c0:c0 + 8, sy, sx])
    return y


# ---- guarded device buffers (GPU tests only)
GUARD_ROWS = 256
SENTINEL = 777.0
PITCHES = ('dense', '+8', '+24', 'slice')


def pitch_of(C, kind):
    """(pitch, offset) in elements of a C-channel operand: dense, 8 or 24 spare lanes, or a channel slice at offset 8 of a buffer
    twice as wide.  C is rounded up to 8 first: rows stay 16-byte addressable."""
    C8 = (C + 7) // 8 * 8
    if kind == 'packed':          # exactly C lanes: rows of an odd width are not 16-byte aligned (outputs and weights only)
        return C, 0
    if kind == 'dense':
        return C8, 0
    if kind == 'slice':
        return 2 * C8 + 8, 8
    return C8 + int(kind), 0


class Guarded(object):
    """one flat device tensor [guard | rows x pitch | guard] (guards of 256 rows); `.view` is the (rows, C) operand inside it, whose
    data_ptr() is what a launch receives.  Inputs: NaN everywhere outside the operand (`zero_to`: zeros in lanes [C, zero_to), the
    lanes a data gradient contracts over).  Outputs: the sentinel everywhere; after the launch `untouched()` says whether every
    element outside the operand still holds its bits."""

    def __init__(self, rows, C, kind='dense', dtype=torch.float16, values=None, zero_to=0, device=None):
        from gpu_util import dev
        self.rows, self.C = rows, C
        self.pitch, self.offset = pitch_of(max(C, zero_to), kind)
        fill = SENTINEL if values is None else float('nan')
        self.flat = torch.full(((2 * GUARD_ROWS + rows) * self.pitch,), fill, dtype=dtype, device=device or dev())
        body = self.flat[GUARD_ROWS * self.pitch:(GUARD_ROWS + rows) * self.pitch].view(rows, self.pitch)
        self.view = body[:, self.offset:self.offset + C]
        if values is not None:
            if zero_to > C:
                body[:, self.offset + C:self.offset + zero_to] = 0
            self.view.copy_(torch.from_numpy(np.array(values, dtype=np.float64)).to(self.flat.device))
        assert self.view.data_ptr() % 16 == 0

    def result(self):
        """host copy of the operand"""
        return self.view.cpu().numpy()

    def untouched(self):
        """True when everything outside the operand is bit-identical to the sentinel (the operand is overwritten by the check)"""
        self.view.fill_(SENTINEL)
        return bool((self.flat == SENTINEL).all().item())


# ---- the siblings: grouped, depthwise and packed-stem convolutions through the same operands and conditions
@functools.lru_cache(maxsize=None)
def grouped_problem(N, C, O, groups, H, W, K, s, p, d):
    """operands and float64 references of a grouped (groups == C == O: depthwise) convolution; weights (O, C / groups, K, K)"""
    Cg = C // groups
    for salt in range(16):
        rs = np.random.RandomState(case_seed((N, C, O, groups, H, W, K, s, p, d), salt))
        q = Problem()
        q.case, q.salt = (N, C, O, groups, H, W, K, s, p, d), salt
        q.x = int_operand(rs, (N, C, H, W), -3, 3)
        q.w = masked_weights(rs, (O, Cg, K, K), Cg * K * K / 2.0 ** salt)
        xt, wt = torch.from_numpy(q.x).requires_grad_(True), torch.from_numpy(q.w).requires_grad_(True)
        y = Fnn.conv2d(xt, wt, None, s, p, d, groups=groups)
        q.dy = int_operand(rs, tuple(y.shape), -3, 3)
        y.backward(torch.from_numpy(q.dy))
        q.y, q.dx, q.dw = y.detach().numpy() + 0.0, xt.grad.numpy() + 0.0, wt.grad.numpy() + 0.0
        q.bias = int_operand(rs, (O,), -8, 8)
        q.acc = int_operand(rs, q.x.shape, -8, 8)
        q.dw0 = int_operand(rs, q.w.shape, -8, 8)
        q.y_br = np.maximum(q.y + q.bias.reshape(1, O, 1, 1), 0.0)
        q.dx_acc = q.dx + q.acc
        if float((q.y == 0).mean()) <= MAX_ZERO_SHARE:
            break
    for name in ('x', 'w', 'dy', 'y', 'y_br', 'dx', 'dx_acc', 'dw', 'dw0'):
        a = getattr(q, name)
        assert np.all(np.round(a) == a) and np.abs(a).max() <= FP16_EXACT, (q.case, name)
        a.setflags(write=False)
    assert float((q.y == 0).mean()) <= MAX_ZERO_SHARE, (q.case, 'zero share', float((q.y == 0).mean()))
    return q
