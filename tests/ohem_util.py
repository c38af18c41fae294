"""What the BoxAnnotatorOHEM tests share: a float64 restatement of lib/operator_py/box_annotator_ohem.py:27-78 and the inputs of
the kernel cases.

The restatement fixes the order where numpy's is unspecified, the way include/sniper_hip.h states it: RoIs rank by descending
loss, equal losses by ascending RoI index (np.argsort(-loss, kind='stable')), a NaN loss first (mapped to +inf).

Equality with an fp32 kernel is meaningful only where no two losses at the selection boundary are closer than the fp32 error of
the loss: fp32 and float64 losses differ by a few 1e-7 relative (an 81-term log-sum-exp), so a case is accepted only if in every
image the k-th and (k+1)-th largest valid losses differ by more than 1e-4 * max(1, loss) -- >= 100 x that error -- and, where an
image has no more than k valid RoIs, its smallest valid loss is that far above the 0 of the ignored RoIs.  Each case takes the
first seed, from 0 upward, that passes (tests/test_ohem_cases_cpu.py asserts the condition for every case the GPU test uses)."""
import functools

import numpy as np

GAP = 1e-4


def losses(cls_score, bbox_pred, labels, bbox_targets, bbox_weights):
    """(B, R) float64: valid ? -log(softmax(score)[label] + 1e-14) + sum_j w_j * smooth_l1(pred_j - target_j) : 0"""
    s = np.asarray(cls_score, np.float64)
    lab = np.asarray(labels, np.float64)
    C = s.shape[-1]
    valid = lab >= 0
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        z = s - s.max(-1, keepdims=True)
        p = np.exp(z) / np.exp(z).sum(-1, keepdims=True)
        li = np.clip(np.where(valid, lab, 0), 0, C - 1).astype(np.int64)      # a label >= C: the reference's index after clipping
        cls = -np.log(np.take_along_axis(p, li[..., None], -1)[..., 0] + 1e-14)
        d = np.asarray(bbox_pred, np.float64) - np.asarray(bbox_targets, np.float64)
        sl1 = np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
        box = (np.asarray(bbox_weights, np.float64) * sl1).sum(-1)
    return np.where(valid, cls + box, 0.0)


def ohem_reference(cls_score, bbox_pred, labels, bbox_targets, bbox_weights, k):
    """-> labels_ohem (B, R), bbox_weights_ohem (B, R, box_dim), fg_labels (B, R), float32"""
    loss = losses(cls_score, bbox_pred, labels, bbox_targets, bbox_weights)
    lab = np.asarray(labels, np.float32)
    lab_out = np.where(lab >= 0, lab, np.float32(-1)).astype(np.float32)      # :56 writes -1 over every label < 0
    w_out = np.array(bbox_weights, np.float32, copy=True)
    for i in range(lab.shape[0]):
        key = np.where(np.isnan(loss[i]), np.inf, loss[i])
        order = np.argsort(-key, kind='stable')
        drop = order[k:]
        lab_out[i, drop] = -1
        w_out[i, drop] = 0
    fg = np.where(lab_out == 0, np.float32(-1), lab_out).astype(np.float32)
    return lab_out, w_out, fg


def gap_ok(loss, labels, k):
    """the acceptance condition of the module docstring, for one case"""
    for i in range(loss.shape[0]):
        v = np.sort(loss[i][labels[i] >= 0])[::-1]
        if not np.isfinite(v).all():
            return False
        if k >= loss.shape[1] or v.size == 0:
            continue
        if v.size > k:
            if not v[k - 1] - v[k] > GAP * max(1.0, v[k - 1]):
                return False
        elif not v[-1] > GAP:
            return False
    return True


def draw(rs, B, R, C, box_dim=4, ignored=None, sparse=None):
    """Inputs as the acceptance test draws them: labels -1 at 20 %, background at 40 %, the foreground classes share the rest;
    weights nonzero only on foreground.  `ignored`: an image whose labels are all -1; `sparse` = (image, n): only its first n
    labelled RoIs stay labelled."""
    pr = [0.2, 0.4] + [0.4 / (C - 1)] * (C - 1)
    lab = rs.choice(np.arange(-1, C), size=(B, R), p=pr).astype(np.float32)
    if ignored is not None:
        lab[ignored] = -1
    if sparse is not None:
        img, n = sparse
        idx = np.flatnonzero(lab[img] >= 0)
        lab[img, idx[n:]] = -1
    score = (rs.standard_normal((B, R, C)) * 2).astype(np.float32)
    pred = rs.standard_normal((B, R, box_dim)).astype(np.float32)
    tgt = rs.standard_normal((B, R, box_dim)).astype(np.float32)
    wgt = np.repeat((lab > 0).astype(np.float32)[:, :, None], box_dim, 2)
    return score, pred, lab, tgt, wgt


# (B, R, C, k, box_dim, ignored image, (sparse image, labelled RoIs left))
CASES = {
    'small': (1, 24, 5, 7, 4, None, None),
    'wave_plus_one_k1': (3, 65, 2, 1, 4, 1, None),                 # R one past a wave, k = 1; image 1 all ignored
    'launch_geometry': (2, 300, 81, 128, 4, None, (1, 50)),        # C > 64 and no multiple of it; image 1: fewer valid than k
    'k_equals_r': (2, 300, 81, 300, 4, None, None),
    'k_beyond_r': (2, 300, 81, 1000, 4, None, None),
    'upper_range': (1, 6000, 21, 256, 4, None, None),              # RPN_PRE_NMS_TOP_N RoIs in one image
    'box_dim_8': (2, 64, 81, 16, 8, None, (0, 5)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (inputs (score, pred, labels, targets, weights), k, expected (labels_ohem, weights_ohem, fg_labels), seed).  Computed once
    per process; callers do not modify the arrays."""
    B, R, C, k, box_dim, ignored, sparse = CASES[name]
    for seed in range(1000):
        ins = draw(np.random.RandomState(seed), B, R, C, box_dim, ignored, sparse)
        if gap_ok(losses(*ins), ins[2], k):
            for a in ins:
                a.setflags(write=False)
            return ins, k, ohem_reference(*ins, k), seed
    raise AssertionError('no seed below 1000 gives case %s a selection boundary wider than %g' % (name, GAP))
