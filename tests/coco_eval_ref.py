"""A restatement of the reference's COCO box evaluation in plain Python and numpy: COCOeval.evaluateImg, accumulate and summarize
(lib/dataset/pycocotools/cocoeval.py:163-272, 312-365, 376-427) and bbIou (lib/dataset/pycocotools/maskApi.c:98-109).  It depends
neither on the kernels nor on the reference; tests/golden/cocoeval_v1.npz (written from the reference itself) pins it on the bits,
and it in turn is what the device is compared with where no golden exists.

Layout shared by the goldens, this file and the kernels.  A PROBLEM is a (category, image) pair with a detection or a box; problems
are ordered category-major, then by image.  Inside a problem, boxes and detections keep the order of the input arrays ("arrival
order" = ascending annotation id).  With NK = sum over problems of min(D_p, maxDets[-1]):
    dt_perm (ND), gt_perm (NG)     input row of every CSR row;  dt_off, gt_off, kp_off (P+1);  cat_off (K+1);  prob_cat, prob_img (P)
    dt_rank (NK)                   arrival index (within its problem) of the r-th kept detection;  dt_scores (NK)
    dt_match (A,T,NK) int32        1 + arrival index of the matched box within the problem, 0 = unmatched
    dt_ignore (A,T,NK) uint8;  gt_match (A,T,NG) int32 = 1 + rank of the matching detection;  gt_ignore (A,NG) uint8
    precision (T,R,K,A,M), recall (T,K,A,M), stats (12,)

`defect` plants one wrong reading of the reference (tests/test_coco_eval_cpu.py shows that the goldens notice each):
    'first_of_equal'  a box of equal IoU does not replace the best so far      'gt_threshold'  IoU > t instead of >= t
    'exclusive_area'  an area equal to a bound lies outside the range          'unstable_ties' equal scores in reverse arrival order
    'no_crowd_rematch' a matched crowd box is skipped like any other
"""
from collections import defaultdict

import numpy as np

EPS = 2.220446049250313e-16          # np.spacing(1)


class Params(object):
    """cocoeval.py:436-445 (box evaluation, per category)"""

    def __init__(self):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]


def bb_iou(d, g, crowd):
    """bbIou for one pair of xywh boxes (Python floats: two roundings in da+ga-i, no fused multiply-add)"""
    ga = g[2] * g[3]
    da = d[2] * d[3]
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    if w <= 0:
        return 0.0
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = da if crowd else da + ga - i
    return i / u


def group(gt, dt, K):
    """-> [(k, i, [gt rows], [dt rows])] category-major, then by image, for every pair that has anything"""
    g, d = defaultdict(list), defaultdict(list)
    for n in range(len(gt['image'])):
        g[int(gt['category'][n]), int(gt['image'][n])].append(n)
    for n in range(len(dt['image'])):
        d[int(dt['category'][n]), int(dt['image'][n])].append(n)
    keys = sorted(set(g) | set(d))
    assert all(0 <= k < K for k, _ in keys)
    return [(k, i, g.get((k, i), []), d.get((k, i), [])) for k, i in keys]


def _outside(area, lo, hi, defect):
    if defect == 'exclusive_area':
        return area <= lo or area >= hi
    return area < lo or area > hi


def evaluate_img(gt, dt, gi, di, params, defect=None):
    """one problem -> order (kept arrival indices), dtm (A,T,D), dtig (A,T,D), gtm (A,T,G), gtig (A,G); ids as in the module docstring"""
    T, A, max_det = len(params.iouThrs), len(params.areaRng), params.maxDets[-1]
    scores = [float(dt['score'][n]) for n in di]
    if defect == 'unstable_ties':
        order = sorted(range(len(di)), key=lambda r: (-scores[r], -r))[:max_det]
    else:
        order = sorted(range(len(di)), key=lambda r: -scores[r])[:max_det]            # stable: equal scores by arrival
    D, G = len(order), len(gi)
    gbox = [[float(v) for v in gt['bbox'][n]] for n in gi]
    dbox = [[float(v) for v in dt['bbox'][di[r]]] for r in order]
    crowd = [int(gt['iscrowd'][n]) for n in gi]
    ious = [[bb_iou(dbox[r], gbox[g], crowd[g]) for g in range(G)] for r in range(D)]
    dtm = np.zeros((A, T, D), np.int32)
    dtig = np.zeros((A, T, D), np.uint8)
    gtm = np.zeros((A, T, G), np.int32)
    gtig = np.zeros((A, G), np.uint8)
    for a, (lo, hi) in enumerate(params.areaRng):
        ig = [1 if (crowd[g] == 1 or int(gt['ignore'][gi[g]]) or _outside(float(gt['area'][gi[g]]), lo, hi, defect)) else 0
              for g in range(G)]
        gtig[a] = ig
        gtind = sorted(range(G), key=lambda g: ig[g])                                  # ignored boxes last, each group by arrival
        for t, thr in enumerate(params.iouThrs):
            matched = [0] * G
            for r in range(D):
                iou = min([thr, 1 - 1e-10])
                m = -1
                for g in gtind:
                    if matched[g] > 0 and not (crowd[g] and defect != 'no_crowd_rematch'):
                        continue
                    if m > -1 and ig[m] == 0 and ig[g] == 1:
                        break
                    if defect == 'gt_threshold' and m == -1:
                        if ious[r][g] <= iou:
                            continue
                    elif defect == 'first_of_equal' and m > -1:
                        if ious[r][g] <= iou:
                            continue
                    elif ious[r][g] < iou:
                        continue
                    iou = ious[r][g]
                    m = g
                if m == -1:
                    continue
                dtig[a, t, r] = ig[m]
                dtm[a, t, r] = m + 1
                matched[m] = r + 1
            gtm[a, t] = matched
            for r in range(D):
                if dtm[a, t, r] == 0 and _outside(float(dt['area'][di[order[r]]]), lo, hi, defect):
                    dtig[a, t, r] = 1
    return order, dtm, dtig, gtm, gtig


def evaluate(gt, dt, K, params=None, defect=None):
    """per-image evaluation of every problem -> the flat arrays of the module docstring (no precision / recall yet)"""
    params = params or Params()
    T, A = len(params.iouThrs), len(params.areaRng)
    probs = group(gt, dt, K)
    parts = [evaluate_img(gt, dt, gi, di, params, defect) for _, _, gi, di in probs]
    out = {}
    out['prob_cat'] = np.array([k for k, _, _, _ in probs], np.int32)
    out['prob_img'] = np.array([i for _, i, _, _ in probs], np.int32)
    out['dt_perm'] = np.array([n for _, _, _, di in probs for n in di], np.int64)
    out['gt_perm'] = np.array([n for _, _, gi, _ in probs for n in gi], np.int64)
    off = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out['dt_off'] = off([len(di) for _, _, _, di in probs])
    out['gt_off'] = off([len(gi) for _, _, gi, _ in probs])
    out['kp_off'] = off([len(p[0]) for p in parts])
    out['cat_off'] = np.searchsorted(out['prob_cat'], np.arange(K + 1)).astype(np.int32)
    cat = lambda arrs, shape, dtype: np.concatenate(arrs, axis=-1) if arrs else np.zeros(shape, dtype)
    out['dt_rank'] = cat([np.array(p[0], np.int32) for p in parts], (0,), np.int32).astype(np.int32)
    out['dt_scores'] = np.array([float(dt['score'][di[r]]) for (_, _, _, di), p in zip(probs, parts) for r in p[0]], np.float64)
    out['dt_match'] = cat([p[1] for p in parts], (A, T, 0), np.int32)
    out['dt_ignore'] = cat([p[2] for p in parts], (A, T, 0), np.uint8)
    out['gt_match'] = cat([p[3] for p in parts], (A, T, 0), np.int32)
    out['gt_ignore'] = cat([p[4] for p in parts], (A, 0), np.uint8)
    return out


def accumulate(ev, K, params=None):
    """cocoeval.py:312-365 on the flat arrays -> precision (T,R,K,A,M), recall (T,K,A,M)"""
    params = params or Params()
    T, R, A, M = len(params.iouThrs), len(params.recThrs), len(params.areaRng), len(params.maxDets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    kp, go, co = ev['kp_off'], ev['gt_off'], ev['cat_off']
    for k in range(K):
        p0, p1 = int(co[k]), int(co[k + 1])
        if p0 == p1:
            continue
        pos = np.arange(kp[p0], kp[p1])
        rank = pos - np.repeat(kp[p0:p1], np.diff(kp[p0:p1 + 1]))
        for a in range(A):
            npig = int(np.count_nonzero(ev['gt_ignore'][a, go[p0]:go[p1]] == 0))
            if npig == 0:
                continue
            for m, max_det in enumerate(params.maxDets):
                sel = pos[rank < max_det]
                inds = np.argsort(-ev['dt_scores'][sel], kind='mergesort')
                dtm = ev['dt_match'][a][:, sel][:, inds]
                dtig = ev['dt_ignore'][a][:, sel][:, inds]
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = (tp / (fp + tp + EPS)).tolist()
                    q = [0.0] * R
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    for ri, pi in enumerate(np.searchsorted(rc, params.recThrs)):
                        if pi >= nd:             # the reference's try/except: the loop ends at the first index past the end
                            break
                        q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q
    return precision, recall


SUMMARY_ROWS = ((1, None, 'all', 100), (1, .5, 'all', 100), (1, .75, 'all', 100), (1, None, 'small', 100), (1, None, 'medium', 100),
                (1, None, 'large', 100), (0, None, 'all', 1), (0, None, 'all', 10), (0, None, 'all', 100), (0, None, 'small', 100),
                (0, None, 'medium', 100), (0, None, 'large', 100))


def summarize(precision, recall, params=None):
    """cocoeval.py:376-427 -> stats (12,), the twelve printed lines.  Like the reference, only for the default area ranges and maxDets."""
    params = params or Params()
    stats, lines = np.zeros((12,)), []
    for n, (ap, iou_thr, area, max_dets) in enumerate(SUMMARY_ROWS):
        aind = [i for i, name in enumerate(['all', 'small', 'medium', 'large']) if name == area]
        mind = [i for i, md in enumerate([1, 10, 100]) if md == max_dets]
        if ap == 1:
            s = precision
            if iou_thr is not None:
                s = s[np.where(iou_thr == params.iouThrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        stats[n] = mean_s
        lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6} | maxDets={:>3} ] = {}'.format(
            'Average Precision' if ap == 1 else 'Average Recall', '(AP)' if ap == 1 else '(AR)',
            '%0.2f:%0.2f' % (params.iouThrs[0], params.iouThrs[-1]) if iou_thr is None else '%0.2f' % iou_thr, area, '%d' % max_dets,
            '%.3f' % float(mean_s)))
    return stats, lines


def run(gt, dt, K, params=None, defect=None, summary=True):
    """everything: the flat per-image arrays plus precision, recall and (for the default parameter shapes) stats"""
    params = params or Params()
    ev = evaluate(gt, dt, K, params, defect)
    ev['precision'], ev['recall'] = accumulate(ev, K, params)
    if summary:
        ev['stats'], ev['summary'] = summarize(ev['precision'], ev['recall'], params)
    return ev
