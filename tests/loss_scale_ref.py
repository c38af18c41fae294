"""numpy restatement of dynamic loss scaling (include/sniper_hip.h: sn_grad_guard_scaled, sn_aux_shadow), no device: the finalize --
the guard's eight doubles with the scale divided out, then the scale policy on the scaler's eight doubles -- in float64 statement by
statement as the finalize block computes them, and the shadow of the forward's side effects.  Builds on tests/grad_guard_ref.py."""
import numpy as np

import grad_guard_ref as gref

F32, F64 = np.float32, np.float64
LS_KEYS = ('scale', 'scale_used', 'clean', 'growths', 'backoffs', 'held_max', 'held_min', 'reserved')


def new_ls(init_scale):
    ls = np.zeros(8, F64)
    ls[0] = init_scale
    return ls


def policy(ls, skip, growth_interval, growth_factor, backoff_factor, min_scale, max_scale):
    """-> the scaler's eight doubles after a step that was (skip) or was not skipped: torch.cuda.amp.GradScaler's rule and two clamps"""
    ls = np.asarray(ls, F64).copy()
    S, clean = ls[0], ls[2]
    scale = S
    if skip:
        want = S * F64(backoff_factor)
        scale = max(want, F64(min_scale))
        if scale < S:
            ls[4] += 1.0
        if want < min_scale:
            ls[6] += 1.0
        clean = 0.0
    else:
        clean += 1.0
        if growth_interval > 0 and clean == growth_interval:
            want = S * F64(growth_factor)
            scale = min(want, F64(max_scale))
            if scale > S:
                ls[3] += 1.0
            if want > max_scale:
                ls[5] += 1.0
            clean = 0.0
    ls[0], ls[1], ls[2] = scale, S, clean
    return ls


def guard_scaled(grad, rescale, clip_global_norm, state, ls, growth_interval=2000, growth_factor=2.0, backoff_factor=0.5,
                 min_scale=1.0, max_scale=2.0 ** 24):
    """-> (state, ls): the guard's and the scaler's eight doubles after one sn_grad_guard_scaled over `grad` (fp32, as the arena holds
    it: S times the gradient).  The sum is grad_guard_ref.guard's -- exact whenever every partial sum is an integer below 2^53."""
    S = F64(ls[0])
    base = gref.guard(grad, rescale, None, True, state)            # sumsq, counts and counters: as the plain guard
    sumsq = base[7]
    norm = np.sqrt(sumsq) * abs(F64(F32(rescale))) / S
    clip = F64(F32(clip_global_norm or 0.0))
    c = min(1.0, float(clip / (norm + 1e-6))) if clip > 0 else 1.0
    out = base.copy()
    out[0], out[1] = norm, F64(c) / S
    assert out[2] == (1.0 if out[3] > 0 else 0.0)
    return out, policy(ls, out[2] != 0.0, growth_interval, growth_factor, backoff_factor, min_scale, max_scale)


class Shadow(object):
    """sn_aux_shadow over numpy vectors: records (vector, offset) into one shadow buffer"""

    def __init__(self, vectors, total=None):
        self.vectors = vectors
        self.offs = np.concatenate([[0], np.cumsum([v.size for v in vectors])])[:-1].astype(np.int64)
        self.total = int(sum(v.size for v in vectors))
        self.shadow = np.zeros(total or self.total, F32)

    def save(self):
        for v, o in zip(self.vectors, self.offs):
            self.shadow[o:o + v.size] = v

    def restore(self, state):
        if state[2] != 0.0:
            for v, o in zip(self.vectors, self.offs):
                v[...] = self.shadow[o:o + v.size]
