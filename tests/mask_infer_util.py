"""Shared by the mask-inference tests: the float64 reference of sn_mask_class_prob and its DERIVED error bound.

Reference: from the fp16 VALUES of x and w (the products of two fp16 numbers are exact in float64), with the header's clipping
rule  neg = clip(int(cls), 0, 2K-1),  pos = clip(int(cls) + K, 0, 2K-1).

Bound (derived, not tuned).  A logit is a sum of C exact products and one bias, accumulated in float32 with round-to-nearest,
u = 2^-24: in ANY summation order the error is at most gamma_C * (sum |x w| + |b|) with gamma_C = C u / (1 - C u) <= (C + 2) u for
the channel counts here -- hence e = (C + 2) * 2^-24 * (sum |x w| + |b|) per logit.  The foreground probability
p = 1 / (1 + exp(z_neg - z_pos)) has |dp/dz| = p (1 - p) <= 1/4 in each logit, so the logit errors move it by at most
(e_neg + e_pos) / 4; the softmax's own arithmetic (one subtraction, two exponentials of arguments <= 0, one sum, one reciprocal,
one product, each within a few u of a value <= 1) is covered by the constant 8 * 2^-24:

    |prob - ref| <= (e_neg + e_pos) / 4 + 8 * 2^-24
"""
import numpy as np

U = 2.0 ** -24


def class_rows(cls, K):
    """the two mask_out rows each RoI reads -> (neg (N,), pos (N,)) int64"""
    c = np.asarray(cls, np.float64)
    c = np.trunc(c).astype(np.int64)                    # (int)cls[n]: truncation toward zero
    return np.clip(c, 0, 2 * K - 1), np.clip(c + K, 0, 2 * K - 1)


def mask_logits_ref(x16, w16, bias, cls, K):
    """x16 (N, HW, C), w16 (2K, C) fp16 values (any float dtype holding them), bias (2K,) or None, cls (N,)
    -> (z_neg, z_pos, a_neg, a_pos), each (N, HW) float64: the logits and sum |x w| + |b| of each"""
    x = np.asarray(x16, np.float16).astype(np.float64)
    w = np.asarray(w16, np.float16).astype(np.float64)
    assert x.ndim == 3 and w.shape == (2 * K, x.shape[2])
    b = np.zeros(2 * K) if bias is None else np.asarray(bias, np.float32).astype(np.float64)
    neg, pos = class_rows(cls, K)
    out = []
    for rows in (neg, pos):
        wr = w[rows]                                    # (N, C)
        out.append(np.einsum('npc,nc->np', x, wr) + b[rows][:, None])
    for rows in (neg, pos):
        out.append(np.einsum('npc,nc->np', np.abs(x), np.abs(w[rows])) + np.abs(b[rows])[:, None])
    return tuple(out)


def softmax1(z_neg, z_pos):
    """channel 1 of the 2-way softmax, max subtracted first, in the dtype of the inputs"""
    m = np.maximum(z_neg, z_pos)
    e0, e1 = np.exp(z_neg - m), np.exp(z_pos - m)
    return e1 / (e0 + e1)


def mask_class_prob_ref(x16, w16, bias, cls, K):
    """-> prob (N, HW) float64"""
    zn, zp, _, _ = mask_logits_ref(x16, w16, bias, cls, K)
    return softmax1(zn, zp)


def mask_class_prob_bound(x16, w16, bias, cls, K):
    """-> the elementwise bound on |prob - mask_class_prob_ref| (N, HW) float64 (module docstring)"""
    C = np.asarray(x16).shape[2]
    _, _, an, ap = mask_logits_ref(x16, w16, bias, cls, K)
    return 0.25 * (C + 2) * U * (an + ap) + 8 * U


EDGE_CLASSES = 5


def edge_classes(N, K, rs, start=0):
    """N class indices: 0, K-1 and the out-of-range -1, K, 2K+5 (clipped by the kernel as pick clips them) in rotation from `start`
    for the first ten RoIs, random valid classes after them.  N < 5: call with start = 0, N, 2N, ... to see all five."""
    edge = [0, K - 1, -1, K, 2 * K + 5]
    return np.array([edge[(start + n) % EDGE_CLASSES] if n < 2 * EDGE_CLASSES else rs.randint(0, K) for n in range(N)], np.float32)
