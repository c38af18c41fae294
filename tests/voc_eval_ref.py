"""A restatement of the reference's PASCAL VOC box evaluation in plain Python and numpy: voc_eval and voc_ap
(lib/dataset/pascal_voc_eval.py:116-181, 39-70) on the rows that write_pascal_results (lib/dataset/pascal_voc.py:395-415) writes.
Like the reference it WALKS a class's detections in score order and keeps a `det` flag per box -- it does not use the argument that
makes the device's matching parallel, so agreeing with it is evidence for that argument.  It depends neither on the kernels nor on
the reference; tests/golden/voceval_v1.npz (written from the reference itself) pins it on the bits, and it in turn is what the
device is compared with where no golden exists.  The one thing it adds to the reference: the sort is STABLE (equal scores in
arrival order = class-major, image, row), where the reference's np.argsort(-confidence) leaves their order undefined.

Layout shared by this file and the kernels.  A PROBLEM is a (class, image) pair with a detection or a box; problems are ordered
class-major, then by image.  The detections are given sorted that way (dt['image'], dt['category'], dt['raw'] (n,5) float32 as the
test run holds them, dt['rows'] (n,5) float64 as the result file holds them), so a detection's CSR position is its index.
    gt_perm (NG)                   input row of every CSR box;  dt_off, gt_off (P+1);  cat_off (K+1);  cls_off (K+1) = dt_off[cat_off]
    dt_best (ND) int32             1 + arrival index (within its problem) of the first box of maximal IoU, 0 = none
    dt_iou (ND);  dt_tp, dt_fp (T,ND) uint8;  gt_det (T,NG) int32 = 1 + arrival index of the detection that took the box
    order (ND) int32               CSR positions in every class's sorted order;  rec, prec (T,ND) in that order
    npos (K) int32;  ap07, ap_area (T,K)

`defect` plants one wrong reading of the reference (tests/test_voc_eval_cpu.py shows that the goldens notice each):
    'ge_threshold'   ovmax >= t instead of >                 'last_of_equal'  the last box of equal IoU wins
    'difficult_fp'   a difficult match counts as fp          'second_best'    a detection whose box is taken moves to the next box
    'no_plus_one'    IoU without the + 1                     'unrounded'      the result rows are not rounded
    'unstable_ties'  equal scores in reverse arrival order (the goldens have no equal scores: the tie input notices this one)
"""
from collections import defaultdict

import numpy as np

DEFECTS = ('ge_threshold', 'last_of_equal', 'difficult_fp', 'second_best', 'no_plus_one', 'unrounded', 'unstable_ties')


AP07_THRESHOLDS = np.arange(0., 1.1, 0.1)          # the reference's eleven recall levels, as float64 computes them


def voc_ap(rec, prec, use_07_metric):
    """voc_ap (pascal_voc_eval.py:39-70), restated: the 11-point average of the best precision at recall >= each level, or the area
    under the precision envelope (precision made non-increasing from the right) summed over the recall steps"""
    if use_07_metric:
        total = 0.
        for level in AP07_THRESHOLDS:
            reached = rec >= level
            best = prec[reached].max() if reached.any() else 0
            total += best / 11.
        return total
    envelope = np.maximum.accumulate(np.concatenate((prec, [0.]))[::-1])[::-1]      # envelope[i] = max(prec[i:], 0)
    steps = np.concatenate(([0.], rec, [1.]))
    change = np.flatnonzero(steps[1:] != steps[:-1])
    return np.sum((steps[change + 1] - steps[change]) * envelope[change])


def overlaps(det, boxes, defect=None):
    """IoU of one detection (4,) with the (G,4) boxes of its image in the arithmetic of pascal_voc_eval.py:146-159: widths and
    heights count pixels (+ 1), the two areas are added before the intersection is subtracted, one division"""
    one = 0. if defect == 'no_plus_one' else 1.
    left, top = np.maximum(boxes[:, 0], det[0]), np.maximum(boxes[:, 1], det[1])
    right, bottom = np.minimum(boxes[:, 2], det[2]), np.minimum(boxes[:, 3], det[3])
    common = np.maximum(right - left + one, 0.) * np.maximum(bottom - top + one, 0.)
    det_area = (det[2] - det[0] + one) * (det[3] - det[1] + one)
    box_area = (boxes[:, 2] - boxes[:, 0] + one) * (boxes[:, 3] - boxes[:, 1] + one)
    return common / (det_area + box_area - common)


def layout(gt, dt, K):
    """the CSR offsets of the problems -> dict (module docstring)"""
    g, d = defaultdict(list), defaultdict(list)
    for n in range(len(gt['image'])):
        g[int(gt['category'][n]), int(gt['image'][n])].append(n)
    for n in range(len(dt['image'])):
        d[int(dt['category'][n]), int(dt['image'][n])].append(n)
    keys = sorted(set(g) | set(d))
    assert all(0 <= k < K for k, _ in keys)
    flat = [n for key in keys for n in d.get(key, [])]
    assert flat == list(range(len(dt['image']))), 'the detections must be sorted class-major, image, row'
    off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = {'prob_cat': np.array([k for k, _ in keys], np.int32), 'prob_img': np.array([i for _, i in keys], np.int32),
           'gt_perm': np.array([n for key in keys for n in g.get(key, [])], np.int64),
           'dt_off': off([len(d.get(key, [])) for key in keys]), 'gt_off': off([len(g.get(key, [])) for key in keys])}
    out['cat_off'] = np.searchsorted(out['prob_cat'], np.arange(K + 1)).astype(np.int32)
    out['cls_off'] = out['dt_off'][out['cat_off']]
    return out


def run(gt, dt, K, thresholds=(0.5, 0.7), defect=None):
    """everything (module docstring)"""
    ev = layout(gt, dt, K)
    with np.errstate(divide='ignore', invalid='ignore'):
        return _run(gt, dt, K, thresholds, defect, ev)


def _run(gt, dt, K, thresholds, defect, ev):
    T, ND, NG = len(thresholds), len(dt['image']), len(gt['image'])
    rows = np.asarray(dt['rows'], np.float64)
    if defect == 'unrounded':
        raw = np.asarray(dt['raw'])
        rows = np.concatenate((raw[:, :4].astype(np.float64) + 1, raw[:, 4:5].astype(np.float64)), axis=1)
    prob_of = {(int(k), int(i)): p for p, (k, i) in enumerate(zip(ev['prob_cat'], ev['prob_img']))}
    out = dict(ev)
    out['dt_best'], out['dt_iou'] = np.zeros(ND, np.int32), np.full(ND, -np.inf)
    out['dt_tp'], out['dt_fp'] = np.zeros((T, ND), np.uint8), np.zeros((T, ND), np.uint8)
    out['gt_det'] = np.zeros((T, NG), np.int32)
    out['order'] = np.zeros(ND, np.int32)
    out['rec'], out['prec'] = np.zeros((T, ND)), np.zeros((T, ND))
    out['npos'] = np.zeros(K, np.int32)
    out['ap07'], out['ap_area'] = np.zeros((T, K)), np.zeros((T, K))
    for k in range(K):
        c0, c1 = int(ev['cls_off'][k]), int(ev['cls_off'][k + 1])
        p0, p1 = int(ev['cat_off'][k]), int(ev['cat_off'][k + 1])
        gsel = ev['gt_perm'][ev['gt_off'][p0]:ev['gt_off'][p1]]
        npos = int(np.sum(~(gt['difficult'][gsel] != 0)))
        out['npos'][k] = npos
        confidence = rows[c0:c1, 4]
        if defect == 'unstable_ties':
            sorted_inds = np.array(sorted(range(c1 - c0), key=lambda r: (-confidence[r], -r)), np.int64)
        else:
            sorted_inds = np.argsort(-confidence, kind='stable')            # the reference's sort is not stable: see the module docstring
        out['order'][c0:c1] = c0 + sorted_inds
        nd = c1 - c0
        cand = []                                    # per detection in sorted order: (row, problem, its boxes, overlaps, ovmax, jmax)
        for d in range(nd):
            n = c0 + int(sorted_inds[d])
            p = prob_of[k, int(dt['image'][n])]
            gi = ev['gt_perm'][ev['gt_off'][p]:ev['gt_off'][p + 1]]
            bb = rows[n, :4].astype(float)
            ovmax, jmax, ov = -np.inf, -1, None
            bbgt = gt['bbox'][gi].astype(float).reshape(-1, 4)
            if bbgt.size > 0:
                ov = overlaps(bb, bbgt, defect)
                ovmax = np.max(ov)
                jmax = int(np.argmax(ov))
                if defect == 'last_of_equal':
                    jmax = len(ov) - 1 - int(np.argmax(ov[::-1]))
            out['dt_best'][n], out['dt_iou'][n] = jmax + 1, ovmax
            cand.append((n, p, gi, ov, ovmax, jmax))
        for t, ovthresh in enumerate(thresholds):
            taken = {}                                                           # (problem, box) -> the detection that set det[jmax]
            tp, fp = np.zeros(nd), np.zeros(nd)
            for d in range(nd):
                n, p, gi, ov, ovmax, jmax = cand[d]
                over = ovmax >= ovthresh if defect == 'ge_threshold' else ovmax > ovthresh
                if over and defect == 'second_best' and (p, jmax) in taken:
                    free = [j for j in np.argsort(-ov, kind='stable') if (p, int(j)) not in taken and ov[j] > ovthresh]
                    if free:
                        jmax = int(free[0])
                if over:
                    if not gt['difficult'][gi[jmax]]:
                        if (p, jmax) not in taken:
                            tp[d] = 1.
                            taken[p, jmax] = n
                            out['gt_det'][t, ev['gt_off'][p] + jmax] = n - ev['dt_off'][p] + 1
                        else:
                            fp[d] = 1.
                    elif defect == 'difficult_fp':
                        fp[d] = 1.
                else:
                    fp[d] = 1.
            out['dt_tp'][t, c0 + sorted_inds] = tp.astype(np.uint8)
            out['dt_fp'][t, c0 + sorted_inds] = fp.astype(np.uint8)
            fp = np.cumsum(fp)
            tp = np.cumsum(tp)
            rec = tp / float(npos)
            prec = tp / np.maximum(tp + fp, np.finfo(np.float64).eps)
            out['rec'][t, c0:c1], out['prec'][t, c0:c1] = rec, prec
            out['ap07'][t, k] = voc_ap(rec, prec, True)
            out['ap_area'][t, k] = voc_ap(rec, prec, False)
    return out


def summary(ap, class_names, use_07_metric, thresholds=(0.5, 0.7)):
    """the text do_python_eval returns (pascal_voc.py:417-456): the metric line, then per threshold one line per class and the mean,
    a blank line between the thresholds and no newline at the end"""
    parts = ['VOC07 metric? %s\n' % ('Y' if use_07_metric else 'No')]
    for t, thr in enumerate(thresholds):
        for k, name in enumerate(class_names):
            parts.append('AP for %s = %.4f\n' % (name, ap[t, k]))
        parts.append('Mean AP@%g = %.4f' % (thr, np.mean([ap[t, k] for k in range(len(class_names))])))
        if t + 1 < len(thresholds):
            parts.append('\n\n')
    return ''.join(parts)
