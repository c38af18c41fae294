"""Exact-arithmetic oracle of the small kernels ("Exact tests of the small kernels"): pooling, element-wise and clip,
layout conversion, weight transposes, smooth-L1, SGD, depth <-> space, pick, sn_copy2d.

Operands are small integers or dyadic fractions, chosen so that every product, sum and stored value is exactly representable where
the kernel holds it (fp32 in registers, fp16 or fp32 in memory): the result does not depend on evaluation order or on what the
compiler contracts, and the comparison is on the bits.  Three roundings cannot be avoided -- the fp32 -> fp16 stores, the one
division of the average pool, `ad - 0.5f * th` of smooth-L1 under sigma = 3 -- and there the operand of the rounding is exact, so
the reference is "float64, rounded once".  This module holds what the CPU test (test_small_ops_cases_cpu.py) and the GPU tests
(test_gpu_small_ops_exact.py) share: the case lists, the operands, the float64 references, the conditions each problem is built
under (check_exact) and the bit comparison.  No device work happens here."""
import functools
import os
import re

import numpy as np
import torch
import torch.nn.functional as Fnn

from bn_exact_util import Counts, kinds  # noqa: F401
from conv_exact_util import PITCHES, SENTINEL, Guarded, case_seed, exact_equal, first_mismatch, pitch_of  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sniper_amd', 'csrc')

# items one launch covers before a thread takes a second trip of its grid-stride loop (blocks x 256 threads)
EW_CAP_ITEMS = 8192 * 256       # csrc/nn_ops.hip:408  `static int ew_blocks(long total) { return sn_blocks(total, 8192); }`
DS_CAP_ITEMS = 16384 * 256      # csrc/mask.hip:107 and :118  `if (blocks > 16384) blocks = 16384;` (depth_to_space2, space_to_depth2)
BEYOND = 257                    # the large cases: cap + one block + one item

POISON16 = 60000.0              # finite, an fp16 value, above every operand: it wins a max, passes a ReLU, leaves a clip at `hi`
F16, F32, F64 = np.float16, np.float32, np.float64


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def source_caps():
    """the grid caps as the sources spell them, in items: {'ew', 'dw' (sn_clip_f16 launches on dwconv.hip's dw_blocks), 'ds'}"""
    ew = re.findall(r'static int ew_blocks\(long total\) \{ return sn_blocks\(total, (\d+)\); \}', _src('nn_ops.hip'))
    dw = re.findall(r'static int dw_blocks\(long total\) \{ return sn_blocks\(total, (\d+)\); \}', _src('dwconv.hip'))
    ds = re.findall(r'if \(blocks > (\d+)\) blocks = (\d+);', _src('mask.hip'))
    assert len(ew) == 1 and len(dw) == 1, (ew, dw)
    assert len(ds) == 2 and len(set(ds[0] + ds[1])) == 1, ds          # both entry points, one literal
    return {'ew': int(ew[0]) * 256, 'dw': int(dw[0]) * 256, 'ds': int(ds[0][0]) * 256}


def clip_cap_items():
    return source_caps()['dw']


# ---- problems
class Prob(object):
    """One problem: arrays as attributes.  `stored[name]` is the type the named array lives in on the device and must survive
    unchanged; `rounded[name] = (exact, dtype, how)`: the named array is `exact` (itself exact in fp32, the register type) rounded
    once to `dtype`."""

    def __init__(self, case):
        self.case, self.stored, self.rounded = case, {}, {}

    def put(self, name, arr, dtype):
        setattr(self, name, arr)
        self.stored[name] = dtype
        return arr

    def put_rounded(self, name, exact, dtype, how):
        setattr(self, name, exact.astype(dtype))
        self.rounded[name] = (exact, dtype, how)
        return getattr(self, name)

    def freeze(self):
        for v in vars(self).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        return self


def survives(a, dtype):
    """every element is finite and a value of `dtype`"""
    a = np.asarray(a)
    with np.errstate(over='ignore'):
        b = a.astype(dtype)
    return bool(np.isfinite(b).all() and np.array_equal(b, a))            # (the comparison promotes: exact)


def check_exact(q):
    """what the zero tolerance rests on, asserted on the problem alone"""
    assert q.stored, q.case
    for name, dt in q.stored.items():
        assert survives(getattr(q, name), dt), (q.case, name, 'is not exact in', np.dtype(dt).name)
    for name, (exact, dt, how) in q.rounded.items():
        assert survives(exact, F32), (q.case, name, 'the operand of the rounding is not exact in fp32', how)
        assert first_mismatch(getattr(q, name), exact.astype(dt)) is None, (q.case, name, how)


def _rs(case, salt=0):
    return np.random.RandomState(case_seed(case, salt))


def _big(n):
    return n > (1 << 20)


def ints(rs, shape, lo, hi, big=False):
    """integers in [lo, hi]: float64, or (the large cases: a quarter of the host memory) float32"""
    return rs.randint(lo, hi + 1, size=shape, dtype=np.int16).astype(F32 if big else F64)


def compare(got, want, what):
    """'' when `got` has the bits of `want` (float64, cast to got's type), else a message naming the first differing element"""
    bad = first_mismatch(got, want)
    if bad is None:
        return ''
    got, want = np.asarray(got), np.asarray(want)
    n_bad = int((got.astype(F64) != want.astype(F64)).sum())
    return '%s: %d of %d elements differ (NaN counted); first %r: got %r want %r' % (what, n_bad, want.size, bad, float(got[bad]), float(want[bad]))


# ---------------------------------------------------------------------------------------------------- sn_ew_f16 / sn_clip_f16
EW_C, EW_ROWS = (8, 24, 72), (1, 7, 257)
EW_LARGE = (EW_CAP_ITEMS + BEYOND, 8)
CLIP_BOUNDS = ((0.0, 6.0), (-2.0, 3.0))


def ew_cases():
    """(rows, C)"""
    return tuple((r, c) for c in EW_C for r in EW_ROWS) + (EW_LARGE,)


def clip_cases():
    return tuple((r, c) for c in EW_C for r in EW_ROWS) + ((clip_cap_items() + BEYOND, 8),)


@functools.lru_cache(maxsize=4)
def ew_problem(case):
    """a, b in [-8, 8], ref in [-2, 2] (two fifths of it on or below the ReLU edge): every sum is an integer of magnitude <= 16"""
    rows, C = case
    rs, big = _rs(case), _big(rows * C)
    q = Prob(case)
    a, b = q.put('a', ints(rs, (rows, C), -8, 8, big), F16), q.put('b', ints(rs, (rows, C), -8, 8, big), F16)
    ref = q.put('ref', ints(rs, (rows, C), -2, 2, big), F16)
    q.put('relu', np.maximum(a, 0), F16)
    q.put('add', a + b, F16)
    q.put('bwd', np.where(ref > 0, a, 0), F16)
    q.put('bwd_b', q.bwd + b, F16)
    return q.freeze()


@functools.lru_cache(maxsize=4)
def clip_problem(case, bounds):
    """a in [-9, 9], ref in [-4, 8] -- exactly on lo and on hi about once in 13 each --, acc in [-8, 8]"""
    rows, C = case
    lo, hi = bounds
    rs, big = _rs(case + bounds), _big(rows * C)
    q = Prob(case + bounds)
    a, ref = q.put('a', ints(rs, (rows, C), -9, 9, big), F16), q.put('ref', ints(rs, (rows, C), -4, 8, big), F16)
    acc = q.put('acc', ints(rs, (rows, C), -8, 8, big), F16)
    q.put('fwd', np.clip(a, lo, hi), F16)
    q.put('bwd', np.where((ref >= lo) & (ref <= hi), a, 0), F16)
    q.put('bwd_acc', q.bwd + acc, F16)
    return q.freeze()


def as_buffer(values, C, kind, fill):
    """host image of conv_exact_util.Guarded's body for an operand: (rows, pitch) of `fill` with the values at the kind's offset"""
    pitch, off = pitch_of(C, kind)
    body = np.full((values.shape[0], pitch), fill, F64)
    body[:, off:off + C] = values
    return body, pitch, off


def read_at_pitch(body, off, C, rows, pitch):
    """the (rows, C) operand a kernel would see that walked `body` at `pitch` instead of the body's own (reads past the end: NaN)"""
    flat = np.concatenate([body.ravel(), np.full(rows * pitch + C, np.nan)])
    idx = off + np.arange(rows)[:, None] * pitch + np.arange(C)[None, :]
    return flat[idx]


# ------------------------------------------------------------------------------------------------------------- sn_maxpool_fwd
POOL_GEOMS = ((3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 2, 0))
POOL_HW = ((7, 6), (6, 7), (8, 5), (3, 4), (1, 1))      # odd / even mixes; 7 under 3/2/1: the last window is cut by the border
POOL_C = (8, 24)
POOL_LARGE = (1, 2898, 2898, 8, 3, 2, 1)                # 1449 x 1449 = 2 099 601 output chunks
POOL_RING = 2                                           # pixels this close to the border are negative


def pool_out(H, k, s, p):
    return (H + 2 * p - k) // s + 1 if H + 2 * p >= k else 0


def pool_cases():
    """(N, H, W, C, k, s, p)"""
    out = [(2, H, W, C, k, s, p) for (k, s, p) in POOL_GEOMS for (H, W) in POOL_HW for C in POOL_C
           if pool_out(H, k, s, p) > 0 and pool_out(W, k, s, p) > 0]
    return tuple(out) + (POOL_LARGE,)


def pool_ref(x_nhwc, k, s, p, pad_value=None):
    """torch-CPU max_pool2d of (N, H, W, C) float32, channels-last in and out; pad_value: the window also sees a border of that
    value (what a kernel computes that lets its padding taps contribute)"""
    t = torch.from_numpy(x_nhwc if x_nhwc.flags.writeable else x_nhwc.copy()).permute(0, 3, 1, 2)
    if pad_value is not None:
        t, p = Fnn.pad(t, (p, p, p, p), value=float(pad_value)), 0
    return np.ascontiguousarray(Fnn.max_pool2d(t, k, s, p).permute(0, 2, 3, 1).numpy())


@functools.lru_cache(maxsize=2)
def pool_problem(case):
    """integers in [-9, 9], all negative within POOL_RING pixels of the border: a padding tap that contributed 0 would win every
    border window"""
    N, H, W, C, k, s, p = case
    rs = _rs(case)
    x = rs.randint(-9, 10, size=(N, H, W, C), dtype=np.int16).astype(F32)
    ring = np.minimum.outer(np.minimum(np.arange(H), H - 1 - np.arange(H)), np.minimum(np.arange(W), W - 1 - np.arange(W))) < POOL_RING
    neg = -rs.randint(1, 10, size=(N, H, W, C), dtype=np.int16).astype(F32)
    x = np.where(ring[None, :, :, None], neg, x)
    q = Prob(case)
    q.put('x', x, F16)
    q.put('y', pool_ref(x, k, s, p), F16)
    return q.freeze()


# ------------------------------------------------------------------------------------------- sn_avgpool_global_fwd / _bwd
AVG_C_N = ((1, (255, 257)), (5, (51, 52)), (81, (3, 4)))       # N * C on both sides of 256
AVG_HW = (1, 49, 64)


def avg_cases():
    """(N, HW, C)"""
    return tuple((N, HW, C) for (C, Ns) in AVG_C_N for HW in AVG_HW for N in Ns)


@functools.lru_cache(maxsize=None)
def avg_problem(case):
    """x in [-8, 8]: the sum over HW <= 64 positions is an integer of magnitude <= 512, exact in fp32 in any order.  Forward:
    float32(s) / float32(HW), ONE correctly rounded division of two exact operands.  Backward: dy an integer in [-64, 64],
    dx = float16(float32(dy) / float32(HW)): the same division, then the fp16 store."""
    N, HW, C = case
    rs = _rs(case)
    q = Prob(case)
    x = q.put('x', ints(rs, (N, HW, C), -8, 8), F16)
    s = q.put('s', x.sum(axis=1), F32)
    q.y = (s.astype(F32) / F32(HW)).astype(F32)
    dy = q.put('dy', ints(rs, (N, C), -64, 64), F32)
    q.quot = (dy.astype(F32) / F32(HW)).astype(F32)
    q.dx = np.broadcast_to(q.quot.astype(F16)[:, None, :], (N, HW, C)).copy()
    q.put('hw', np.array([float(HW)]), F32)
    return q.freeze()


# -------------------------------------------------------------------------------------------------------- sn_transpose_batched
TR_ROWS, TR_COLS = (1, 31, 32, 33, 65), (1, 3, 32, 40, 81)
TR_DTYPES = ((0, 0), (0, 1), (1, 0), (1, 1))               # (in, out), 0 = fp16, 1 = fp32
TR_PADS = (1, 8, 0, 5)                                     # spare elements per row, by rotation
TR_SLACK = (7, 16)                                         # spare elements per batch
NP_OF = {0: F16, 1: F32}


def tr_cases():
    """(batch, rows, cols, in_ld, out_ld, in_batch_stride, out_batch_stride)"""
    out = []
    for i, (r, c) in enumerate((r, c) for r in TR_ROWS for c in TR_COLS):
        in_ld, out_ld = c + TR_PADS[i % 4], r + TR_PADS[(i // 4 + 1) % 4]
        out.append((1 if i % 2 else 3, r, c, in_ld, out_ld, r * in_ld + TR_SLACK[i % 2], c * out_ld + TR_SLACK[(i + 1) % 2]))
    return tuple(out)


def tr_batch(case, pair):
    """batch of a case under a dtype pair: each (shape, pair) runs once, each shape and each pair meets batch 1 and batch 3"""
    return case[0] if TR_DTYPES.index(pair) % 2 == 0 else 4 - case[0]


def tr_values(case, batch, exact):
    """(batch, rows, cols): eighths of magnitude <= 64 (fp16 values), or thirds as fp32 holds them (no fp16 values)"""
    _, r, c = case[:3]
    k = _rs(case, batch).randint(-512, 513, size=(batch, r, c)).astype(F64)
    if exact:
        return k / 8.0
    return (k.astype(F32) / F32(3.0)).astype(F64)


def tr_images(case, batch, values, in_fill, out_fill, out_dtype):
    """host images of the two flat buffers: the input inside `in_fill`, the expected output (rounded once to out_dtype) inside
    `out_fill` -- the spare lanes of both pitches and the slack between batches included"""
    _, r, c, in_ld, out_ld, ibs, obs = case
    src = np.full(batch * ibs, in_fill, F64)
    dst = np.full(batch * obs, out_fill, F64)
    for b in range(batch):
        src[b * ibs:b * ibs + r * in_ld].reshape(r, in_ld)[:, :c] = values[b]
        dst[b * obs:b * obs + c * out_ld].reshape(c, out_ld)[:, :r] = values[b].T.astype(out_dtype).astype(F64)
    return src, dst


# ------------------------------------------------------------------------- sn_weight_transpose / sn_weight_transpose_batched
WT_SHAPES = ((1, 1, 1, 8), (65, 9, 63, 72), (40, 9, 24, 40), (512, 9, 512, 512))       # (O, T, I, Opad); the last: 2 359 296 items
WT_TABLE = (0, 3, 1, 2, 0)            # the batched table, as indices into WT_SHAPES: small first and last, the large one inside


@functools.lru_cache(maxsize=None)
def wt_problem(shape):
    """fp32 [O][T][I] of eighths (fp16 values) -> fp16 [I][T][Opad], zero in columns O..Opad-1"""
    O, T, I, Opad = shape
    q = Prob(shape)
    w = q.put('w', _rs(shape).randint(-512, 513, size=(O, T, I)).astype(F64) / 8.0, F16)
    wt = np.zeros((I, T, Opad))
    wt[:, :, :O] = w.transpose(2, 1, 0)
    q.put('wt', wt, F16)
    return q.freeze()


WT_DESC = np.dtype([('src', '<u8'), ('dst', '<u8'), ('O', '<i4'), ('T', '<i4'), ('I', '<i4'), ('Opad', '<i4'), ('tile0', '<i4'),
                    ('tiles_o', '<i4'), ('tiles_i', '<i4'), ('pad', '<i4')])        # csrc/nn_ops.hip WtDesc, 48 bytes


def wt_table(shapes, src_ptrs, dst_ptrs):
    """-> (descriptor records, total tiles): weight k owns T * ceil(Opad / 64) * ceil(I / 64) tiles of 64 x 64"""
    rec = np.zeros(len(shapes), WT_DESC)
    tile0 = 0
    for k, ((O, T, I, Opad), s, d) in enumerate(zip(shapes, src_ptrs, dst_ptrs)):
        to, ti = (Opad + 63) // 64, (I + 63) // 64
        rec[k] = (s, d, O, T, I, Opad, tile0, to, ti, 0)
        tile0 += T * to * ti
    return rec, tile0


# ---------------------------------------------------------------------------------------------------------- sn_smooth_l1_loss
SL1_N = (1, 255, 256, 257, EW_CAP_ITEMS + BEYOND)
SL1_SIGMA = (1.0, 3.0)
SL1_W = (0.0, 0.5, 1.0, 2.0)
SL1_GRAD_SCALE = 0.25


def sl1_cases():
    """(n, sigma)"""
    return tuple((n, s) for s in SL1_SIGMA for n in SL1_N)


@functools.lru_cache(maxsize=4)
def sl1_problem(case):
    """d = pred - target in 64ths: half of them |d| <= 12/64 (both sides of 1/9, 0 included), the rest up to 8; pred and target
    64ths of magnitude < 16.  s2 = sigma^2 in {1, 9}, th = float32(1 / s2).  Quadratic branch: 0.5 s2 d^2 = s2 m^2 / 8192, an
    integer below 2^16 over a power of two.  Linear branch: |d| - 0.5 th, exact under sigma = 1; under sigma = 3 th is no dyadic
    number and the difference is rounded ONCE (0.5 th is exact, so a fused multiply-subtract rounds the same value).  w and
    grad_scale are powers of two or zero."""
    n, sigma = case
    rs = _rs(case)
    q = Prob(case)
    m = np.where(rs.random_sample(n) < 0.5, rs.randint(-12, 13, size=n), rs.randint(-512, 513, size=n)).astype(F64)
    if n >= 255:
        m[:3] = (0.0, 7.0, -8.0)           # 7/64 < 1/9 < 8/64
    t = rs.randint(-256, 257, size=n).astype(F64)
    pred, target = q.put('pred', (t + m) / 64.0, F32), q.put('target', t / 64.0, F32)
    w = q.put('w', rs.choice(SL1_W, size=n), F32)
    d = q.put('d', pred - target, F32)
    s2 = sigma * sigma
    th = F64(F32(1.0) / F32(s2))
    q.th = float(th)
    ad = np.abs(d)
    quad = q.put('quad', 0.5 * s2 * d * d, F32)
    q.put('half_th', np.array([0.5 * th]), F32)
    lin_exact = ad - 0.5 * th                                   # float64: exact (both operands within 2^-30 .. 2^4)
    lin = lin_exact.astype(F32).astype(F64)
    q.lin_exact, q.lin = lin_exact, lin
    q.put('loss', w * np.where(ad < th, quad, lin), F32)
    q.put('dpred', SL1_GRAD_SCALE * w * np.where(ad < th, s2 * d, np.sign(d)), F32)
    q.quadratic = ad < th
    return q.freeze()


# --------------------------------------------------------------------- sn_sgd_mom_update, _dev, _guarded_dev
SGD_HYPER = (2.0 ** -4, 2.0 ** -3, 0.5, 0.25)                 # lr, wd, momentum, rescale
SGD_DEV_HYPER, SGD_MULTS = (2.0 ** -5, 2.0 ** -2, 0.5, 0.25), (2.0, 0.5)       # the device's four floats x (lr_mult, wd_mult): the same
SGD_GUARD = (0.5, 0.25)                                       # the guard's coefficient, the element-wise clip
SGD_N = (1, 2, 3, 4, 5, 1027)
SGD_LARGE_N = 4 * EW_CAP_ITEMS + 4 * BEYOND + 3
SGD_LARGE_OFF = 3               # head 1, body EW_CAP_ITEMS + 257 float4, tail 2
SGD_PAD = 16                    # elements kept on both sides of [off, off + n) (the slice starts at element SGD_PAD + off)
W16_MODES = ('none', 'same', 'half8', 'odd')


def sgd_offsets():
    """start offsets (w32, grad, mom) in {0..3}^3: all equal (the vector path), or exactly one array differing (the fallback)"""
    out = [(o, o, o) for o in range(4)]
    for k in range(3):
        for o in range(4):
            for other in range(4):
                if other != o:
                    t = [o, o, o]
                    t[k] = other
                    out.append(tuple(t))
    return tuple(out)


def sgd_head(ow):
    return (4 - ow) % 4


def w16_offset(ow, mode):
    """element offset of the fp16 copy: 'same' as w32's; 'half8': w16 + head is 8- but not 16-byte aligned (all the vector path
    needs); 'odd': it is not 8-byte aligned (the fallback)"""
    if mode == 'same':
        return ow
    if mode == 'half8':
        return (4 - sgd_head(ow)) % 8
    if mode == 'odd':
        return ow + 1
    return None


def sgd_vector_path(offs, mode):
    """does the head / body / tail split run (else one scalar launch)?  Buffers start 16-byte aligned."""
    ow, og, om = offs
    o16 = w16_offset(ow, mode)
    return ow == og == om and (o16 is None or (o16 + sgd_head(ow)) % 4 == 0)


def sgd_cases():
    """(n, (ow, og, om), w16 mode): every offset combination at every n, the fp16 copy's mode by rotation -- and every mode at every
    n for the combinations that take the vector path"""
    out = []
    for i, offs in enumerate(sgd_offsets()):
        for j, n in enumerate(SGD_N):
            modes = W16_MODES if offs[0] == offs[1] == offs[2] else (W16_MODES[(i + j) % 4],)
            out += [(n, offs, m) for m in modes]
    return tuple(out) + ((SGD_LARGE_N, (SGD_LARGE_OFF,) * 3, 'same'),)


@functools.lru_cache(maxsize=8)
def sgd_problem(n, salt=0):
    """w in eighths (|w| <= 4), grad integers (|g| <= 8), mom in quarters (|m| <= 2): with the dyadic hyper-parameters every term
    of g = rescale * grad + wd * w, mom' = momentum * mom - lr * g, w' = w + mom' is a multiple of 2^-10 of magnitude < 8 -- 13 bits,
    exact in fp32 however the statement is contracted.  The guarded statement's rescale * (coef * grad) = grad / 8, clipped at 1/4,
    is as exact.  The fp16 copy is w' rounded once."""
    big = _big(n)
    rs = _rs((n, 'sgd'), salt)
    q = Prob((n, salt))
    scale = (lambda a, s: a * F32(s)) if big else (lambda a, s: a * s)
    w = q.put('w', scale(ints(rs, (n,), -32, 32, big), 0.125), F32)
    g = q.put('g', ints(rs, (n,), -8, 8, big), F32)
    m = q.put('m', scale(ints(rs, (n,), -8, 8, big), 0.25), F32)
    q.put('h', ints(rs, (n,), -5, 5, big), F16)                       # the fp16 copy on entry
    w, g, m = w.astype(F64), g.astype(F64), m.astype(F64)
    lr, wd, mo, rescale = SGD_HYPER
    coef, clip = SGD_GUARD
    for tag, u in (('', rescale * g), ('_guard', np.clip(rescale * (coef * g), -clip, clip))):
        q.put('u' + tag, u, F32)
        gg = q.put('gg' + tag, u + wd * w, F32)
        nm = q.put('m1' + tag, mo * m - lr * gg, F32)
        nw = q.put('w1' + tag, w + nm, F32)
        q.put_rounded('h1' + tag, nw, F16, 'fp16 copy of the new master weight')
    return q.freeze()


def sgd_image(values, off, fill_rs, lo, hi, step, dtype):
    """an array's host image: SGD_PAD + off elements, the n values, SGD_PAD elements; everything outside the values is a finite
    number of its own (the bits it must keep)"""
    n = values.shape[0]
    img = (fill_rs.randint(lo, hi + 1, size=SGD_PAD + off + n + SGD_PAD) * step).astype(dtype)
    img[SGD_PAD + off:SGD_PAD + off + n] = values.astype(dtype)
    return img


# ------------------------------------------------------------------------------- sn_depth_to_space2 / sn_space_to_depth2
DS_CASES = ((2, 3, 5, 8), (1, 5, 3, 24), (2, 1, 1, 8))        # (N, H, W, C): odd extents
DS_LARGE = (1, 1025, 1025, 8)                                 # 2050 x 2050 = 4 202 500 chunks


def ds_cases():
    return DS_CASES + (DS_LARGE,)


def ds_items(case):
    N, H, W, C = case
    return N * 2 * H * 2 * W * (C // 8)


@functools.lru_cache(maxsize=2)
def ds_problem(case):
    """deep (N, H, W, 4 C) with channel (a * 2 + b) * C + c  <->  space (N, 2 H, 2 W, C); integers in [-9, 9]"""
    N, H, W, C = case
    q = Prob(case)
    deep = q.put('deep', ints(_rs(case), (N, H, W, 4 * C), -9, 9, _big(ds_items(case))), F16)
    space = deep.reshape(N, H, W, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * H, 2 * W, C)
    q.put('space', np.ascontiguousarray(space), F16)
    q.put('space_relu', np.maximum(q.space, 0), F16)
    return q.freeze()


# ------------------------------------------------------------------------------------------------- sn_pick_fwd / sn_pick_bwd
PICK_NHW = ((5, 51), (4, 64), (257, 1))                       # N * HW = 255, 256, 257
PICK_C_FWD, PICK_C_BWD = (5, 8, 24), (8, 24)


def pick_cases(fwd):
    """(N, HW, C)"""
    return tuple((N, HW, C) for (N, HW) in PICK_NHW for C in (PICK_C_FWD if fwd else PICK_C_BWD))


def pick_index(case):
    """per image: below 0, 0, the first / middle / last chunk's channels, C - 1, C and beyond (mx.nd.pick clips)"""
    N, HW, C = case
    base = np.array([-1, C, C // 2, C - 1, 0, C + 3, 3, -7], F64)
    idx = base[np.arange(N) % len(base)]
    if N > len(base):
        idx[len(base):] = _rs(case).randint(-2, C + 2, size=N - len(base))
    return idx


@functools.lru_cache(maxsize=None)
def pick_problem(case):
    N, HW, C = case
    rs = _rs(case)
    q = Prob(case)
    x = q.put('x', ints(rs, (N, HW, C), -9, 9), F16)
    idx = q.put('index', pick_index(case), F32)
    q.clipped = np.clip(idx, 0, C - 1).astype(np.int64)
    q.put('y', np.take_along_axis(x, np.broadcast_to(q.clipped[:, None, None], (N, HW, 1)), axis=2)[:, :, 0], F16)
    dy = q.put('dy', ints(rs, (N, HW), -9, 9), F16)
    dx0 = q.put('dx0', ints(rs, (N, HW, C), -8, 8), F16)
    hot = (np.arange(C)[None, None, :] == q.clipped[:, None, None]) * dy[:, :, None]
    q.put('dx', hot + 0.0, F16)
    q.put('dx_acc', dx0 + hot, F16)
    return q.freeze()


# ------------------------------------------------------------------------------------------------------------------ sn_copy2d
# (rows, cols, in_ld, out_ld, in dtype, out dtype): only what test_copy2d_vectorised_and_scalar_paths lacks -- the element-wise
# kernel (cols % 8 != 0) and the 16-byte kernel on its row / column path (pitches differ), each past the grid cap
COPY_SCALAR = ((EW_CAP_ITEMS + BEYOND + 2) // 3, 3, 5, 4, 1, 0)
COPY_VEC8 = (EW_CAP_ITEMS + BEYOND, 8, 16, 24, 0, 0)


def copy_items(case):
    rows, cols = case[:2]
    return rows * (cols // 8 if cols % 8 == 0 else cols)


@functools.lru_cache(maxsize=2)
def copy_problem(case):
    rows, cols = case[:2]
    q = Prob(case)
    q.put('x', ints(_rs(case), (rows, cols), -2048, 2048, True), F16)
    return q.freeze()
