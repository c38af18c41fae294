"""numpy restatement of gradient accumulation (include/sniper_hip.h: sn_grad_accumulate), no device: the copy /
add of one micro-batch's gradients, and a window driver -- sum in float32 in arrival order, then ONE judgement of the sum by the guard
(tests/grad_guard_ref.py) or the scaled finalize (tests/loss_scale_ref.py), then the restated update on the sum."""
import numpy as np

import grad_guard_ref as gref
import loss_scale_ref as lref

F32, F64 = np.float32, np.float64


def bits(x):
    """float32 array (or scalar) -> its uint32 bit patterns"""
    return np.ascontiguousarray(np.asarray(x, F32)).reshape(-1).view(np.uint32)


def from_bits(b):
    """uint32 bit patterns -> float32 (no conversion instruction touches the value: a subnormal survives whatever mode the host is in)"""
    return np.ascontiguousarray(np.asarray(b, np.uint32)).reshape(-1).view(F32)


def _exact_f64(x):
    """float32 -> float64 through the bit fields, not through a conversion: the host may run with denormals-are-zero (the oracle
    turns torch.set_flush_denormal on for its process), which would read every subnormal float32 as 0.  m * 2^e with m < 2^24 is exact
    in float64 and never subnormal there."""
    b = bits(x)
    e = ((b >> 23) & 0xff).astype(np.int64)
    m = (b & 0x7fffff).astype(np.int64)
    mag = np.ldexp(np.where(e == 0, m, m | 0x800000).astype(F64), np.where(e == 0, -149, e - 150).astype(np.int64))
    with np.errstate(all='ignore'):
        mag = np.where(e == 255, np.where(m == 0, np.inf, np.nan), mag)
    return np.where((b >> 31) == 1, -mag, mag)


def _round_f32(s):
    """float64 -> the nearest float32 (ties to even), subnormal results kept whatever mode the host is in: results below 2^-126 are
    rounded as integers in units of 2^-149 -- which ARE the bit patterns of the subnormals, and of 2^-126 where the rounding carries"""
    with np.errstate(all='ignore'):
        out = s.astype(F32)
        small = (np.abs(s) < 2.0 ** -126) & (s != 0)
    if small.any():
        q = np.rint(np.ldexp(np.abs(s[small]), 149)).astype(np.uint32)            # exact scaling, then round to nearest even
        out.view(np.uint32)[small] = q | (np.signbit(s[small]).astype(np.uint32) << 31)
    return out


def accumulate(acc, grad, first):
    """-> the accumulation arena after one sn_grad_accumulate: first: the bits of grad; else acc + grad, one binary32 addition per
    element (round to nearest even, subnormals kept, inf / NaN propagate).  The sum of two float32 is formed in float64 and rounded
    once: where the exponents are at most 28 apart it is exact in float64; further apart the smaller operand is below 2^-28 of the
    larger, and a float32 rounding boundary is at least 2^-25 of the larger away from it, so both roundings return the larger
    operand.  Nothing here depends on the flush-to-zero mode of the host."""
    g = np.asarray(grad, F32).reshape(-1)
    if first:
        return from_bits(bits(g).copy())
    with np.errstate(all='ignore'):
        return _round_f32(_exact_f64(np.asarray(acc, F32).reshape(-1)) + _exact_f64(g))


def same_bits(got, want):
    """the comparison of the add: bit-equal where want is not NaN, NaN where it is"""
    g, w = bits(got), bits(want)
    is_nan = lambda b: ((b >> 23) & 0xff == 255) & (b & 0x7fffff != 0)
    nan = is_nan(w)
    return bool(g.shape == w.shape and np.array_equal(is_nan(g), nan) and np.array_equal(g[~nan], w[~nan]))


class Window(object):
    """One optimizer over windows of k micro-batches.  hyper = (lr, wd, momentum, rescale) as the device's four floats.  loss_scale:
    None, or a dict of loss_scale_ref.guard_scaled's keyword arguments plus init_scale (the guard is then on with skip_nonfinite).
    aux: vectors a micro-batch's forward rewrites (loss_scale_ref.Shadow saves them before the first micro-step of a window and puts
    them back when the window is skipped)."""

    def __init__(self, k, hyper, lr_mult=1.0, wd_mult=1.0, clip_gradient=None, clip_global_norm=None, skip_nonfinite=False,
                 loss_scale=None, aux=None):
        self.k, self.hyper, self.mults = int(k), tuple(hyper), (lr_mult, wd_mult)
        self.clip_gradient, self.clip_global_norm = clip_gradient, clip_global_norm
        self.skip_nonfinite = bool(skip_nonfinite) or loss_scale is not None
        self.guarded = self.skip_nonfinite or clip_gradient is not None or clip_global_norm is not None
        self.state = np.zeros(8, F64)
        self.policy = None
        if loss_scale is not None:
            self.policy = {key: v for key, v in loss_scale.items() if key != 'init_scale'}
            self.ls = lref.new_ls(loss_scale['init_scale'])
        self.shadow = lref.Shadow(aux) if aux else None
        self.acc, self.pending, self.updates = None, 0, 0

    def scale(self):
        """what the loss kernels of the next micro-batch multiply with: it moves in update() only, so a window carries one scale"""
        return float(self.ls[0]) if self.policy is not None else 1.0

    def before_forward(self):
        if self.pending == 0 and self.shadow is not None:
            self.shadow.save()

    def micro(self, grad):
        self.acc = accumulate(self.acc, grad, self.pending == 0)
        self.pending += 1
        return self.pending

    def update(self, w, mom):
        """-> (w32, mom, w16) after the window's one optimizer pass on whatever is pending"""
        if self.pending == 0:
            raise RuntimeError('nothing pending')
        if self.policy is not None:
            self.state, self.ls = lref.guard_scaled(self.acc, self.hyper[3], self.clip_global_norm, self.state, self.ls, **self.policy)
        elif self.guarded:
            self.state = gref.guard(self.acc, self.hyper[3], self.clip_global_norm, self.skip_nonfinite, self.state)
        state = self.state if self.guarded else [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
        out = gref.guarded_update(w, self.acc, mom, self.hyper, self.mults[0], self.mults[1], self.clip_gradient, state)
        if self.shadow is not None:
            self.shadow.restore(state)
        self.pending = 0
        self.updates += 1
        return out
