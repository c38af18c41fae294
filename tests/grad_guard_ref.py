"""numpy restatement of the gradient guard (include/sniper_hip.h: sn_grad_guard, sn_sgd_mom_update_guarded_dev), no device: the
state in float64 as the finalize block computes it, the update in float32 statement by statement."""
import numpy as np

F32, F64 = np.float32, np.float64
STATE_KEYS = ('norm', 'coef', 'skip', 'nonfinite', 'steps', 'skipped', 'consecutive', 'sumsq')


def finite_mask(grad):
    """non-finite <=> !(|g| <= FLT_MAX)"""
    with np.errstate(invalid='ignore'):
        return np.abs(np.asarray(grad, F32)) <= np.finfo(F32).max


def guard(grad, rescale, clip_global_norm, skip_nonfinite, state):
    """-> the eight doubles after one sn_grad_guard over `grad` (fp32); state: the eight doubles before (zeros at first).  rescale
    and clip_global_norm are taken as the float32 values the device holds.  The sum is numpy's (pairwise) fp64 sum: exact, hence
    equal to the device's, whenever every partial sum is an integer below 2^53; otherwise equal up to the order of summation."""
    g = np.asarray(grad, F32).ravel()
    ok = finite_mask(g)
    bad = int(g.size - int(ok.sum()))
    g64 = g[ok].astype(F64)
    sumsq = F64(np.sum(g64 * g64, dtype=F64))
    norm = np.sqrt(sumsq) * abs(F64(F32(rescale)))
    clip = F64(F32(clip_global_norm or 0.0))
    coef = min(1.0, float(clip / (norm + 1e-6))) if clip > 0 else 1.0
    skip = 1.0 if (skip_nonfinite and bad > 0) else 0.0
    old = np.asarray(state, F64)
    return np.array([norm, coef, skip, bad, old[4] + 1.0, old[5] + skip, old[6] + 1.0 if skip else 0.0, sumsq], F64)


def guarded_update(w, grad, mom, hyper, lr_mult, wd_mult, clip_gradient, state):
    """-> (w32, mom, w16) after sn_sgd_mom_update_guarded_dev; hyper = (lr, wd, momentum, rescale) as the device's four floats, state
    the guard's eight doubles.  Every statement rounds to float32 (no fused multiply-add: the device may contract, one ulp)."""
    w, g, m = (np.asarray(a, F32).copy() for a in (w, grad, mom))
    if state[2] != 0.0:
        return w, m, w.astype(np.float16)
    lr = F32(hyper[0]) * F32(lr_mult)
    wd = F32(hyper[1]) * F32(wd_mult)
    momentum, rescale = F32(hyper[2]), F32(hyper[3])
    coef, clip = F32(state[1]), F32(clip_gradient or 0.0)
    if coef == 1.0 and not clip > 0:
        u = rescale * g
    else:
        u = rescale * (coef * g)
        if clip > 0:
            u = np.minimum(np.maximum(u, -clip), clip)
    gg = u + wd * w
    m = momentum * m - lr * gg
    w = w + m
    return w.astype(F32), m.astype(F32), w.astype(np.float16)
