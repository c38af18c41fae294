"""A restatement of the reference's PASCAL VOC mask evaluation in plain Python and numpy: voc_eval_sds
(lib/dataset/pascal_voc_eval.py:184-272) with mask_overlap (lib/mask/mask_transform.py:40-70) and voc_ap (:39-70, shared with
tests/voc_eval_ref.py).  Like the reference it WALKS a class's detections in score order and keeps an `already_detect` flag per
instance -- it does not use the argument that makes the device's matching parallel, so agreeing with it is evidence for that
argument.  It depends neither on the kernels nor on the reference; tests/golden/vocsds_v1.npz (written from the reference itself,
with tests/coco_segm_ref.py::resize_linear_f32 standing in for cv2.resize) pins its AP on the bits, and it in turn is what the device
is compared with for everything voc_eval_sds does not return.  Two things are this project's: the resize (resize_linear_f32, not
pinned to OpenCV) and the STABLE sort (equal scores in arrival order = class-major, image, row; the reference's np.argsort(-scores)
leaves their order undefined).

A SET is (gt, dt, K, I, M, binary_thresh):
  gt = dict(image, category (0-based), bound (NG,4) x1, y1, x2, y2 as parse_inst gives them, bits (pool,) uint8 -- the cropped boolean
       masks, row-major, one byte per pixel -- and pix_off (NG+1) int64), annotation order;
  dt = dict(image, category, raw (ND,5) float32 rows x1, y1, x2, y2, score, masks (ND,M,M) float32), sorted class-major, image, row.
The layout of the problems is tests/voc_eval_ref.py::layout (the one the box kernels use).  Outputs:
    dt_box (ND,4) int32           np.round(raw[:, :4] in float64).astype(int)
    dt_area (ND) int32            pixels >= float32(binary_thresh) of the resized map
    iou_off (P+1) int32;  iou (n_pairs) float64   problem p's D_p x G_p overlaps at iou_off[p], detection-major
    dt_best (ND) int32            1 + arrival index (within its problem) of the candidate instance, 0 = none
    dt_iou (ND) float64           cur_overlap (-1000 without an instance)
    dt_tp, dt_fp (T,ND) uint8;  gt_det (T,NG) int32 = 1 + arrival index of the detection that took the instance
    order (ND) int32;  rec, prec (T,ND) in sorted order;  npos (K) int32;  ap07 (= what voc_eval_sds returns), ap_area (T,K)

`defect` plants one wrong reading of the reference (tests/test_voc_sds_cpu.py shows that the goldens notice each):
    'strict_threshold'  cur > t instead of >=              'last_of_equal'   the last instance of maximal overlap wins
    'union_plus_inter'  union without `- inter`            'truncated'       astype(int) without np.round
    'thresh_float64'    the map compared in float64        'no_already'      already_detect ignored
    'unstable_ties'     equal scores in reverse arrival order (the goldens have no equal scores: the tie input notices this one)
"""
import numpy as np

import voc_eval_ref as box_ref
from coco_segm_ref import resize_linear_f32

DEFECTS = ('strict_threshold', 'last_of_equal', 'union_plus_inter', 'truncated', 'thresh_float64', 'no_already', 'unstable_ties')

layout = box_ref.layout
voc_ap = box_ref.voc_ap


def gt_mask(gt, n):
    """instance n's boolean mask, shaped by its rounded bound"""
    x1, y1, x2, y2 = np.round(gt['bound'][n]).astype(int)
    lo, hi = int(gt['pix_off'][n]), int(gt['pix_off'][n + 1])
    return gt['bits'][lo:hi].reshape(y2 - y1 + 1, x2 - x1 + 1) != 0


def round_box(row, defect=None):
    """np.round(box).astype(int) on the float64 row (pascal_voc_eval.py:233; new_boxes is a float64 array)"""
    b = np.asarray(row[:4], np.float64)
    return b.astype(int) if defect == 'truncated' else np.round(b).astype(int)


def binarise(mask, box, binary_thresh, defect=None):
    """the map resized to its integer box and thresholded (pascal_voc_eval.py:235-236): float32 >= float32(thresh)"""
    x1, y1, x2, y2 = (int(v) for v in box)
    big = resize_linear_f32(np.asarray(mask, np.float32), y2 - y1 + 1, x2 - x1 + 1)
    if defect == 'thresh_float64':
        return big.astype(np.float64) >= float(binary_thresh)
    return big >= np.float32(binary_thresh)


def mask_overlap(box_a, box_b, mask_a, mask_b, defect=None):
    """mask_transform.py:40-70, restated: the intersection rectangle of the two integer boxes; the pixels set in both inside it over
    the pixels set in either anywhere; 0 for an empty rectangle or an empty union"""
    left, top = max(box_a[0], box_b[0]), max(box_a[1], box_b[1])
    right, bottom = min(box_a[2], box_b[2]), min(box_a[3], box_b[3])
    if left > right or top > bottom:
        return 0
    part_a = mask_a[top - box_a[1]:bottom - box_a[1] + 1, left - box_a[0]:right - box_a[0] + 1]
    part_b = mask_b[top - box_b[1]:bottom - box_b[1] + 1, left - box_b[0]:right - box_b[0] + 1]
    assert part_a.shape == part_b.shape
    common = int(np.logical_and(part_a, part_b).sum())
    either = int(mask_a.sum()) + int(mask_b.sum()) - (0 if defect == 'union_plus_inter' else common)
    if either < 1.0:
        return 0
    return float(common) / float(either)


def run(gt, dt, K, thresholds=(0.5, 0.7), binary_thresh=0.4, defect=None):
    """everything (module docstring)"""
    ev = layout(gt, dt, K)
    with np.errstate(divide='ignore', invalid='ignore'):
        return _run(gt, dt, K, thresholds, binary_thresh, defect, ev)


def _run(gt, dt, K, thresholds, binary_thresh, defect, ev):
    T, ND, NG = len(thresholds), len(dt['image']), len(gt['image'])
    raw = np.asarray(dt['raw'])
    scores = raw[:, 4].astype(np.float64)
    dcount, gcount = np.diff(ev['dt_off']).astype(np.int64), np.diff(ev['gt_off']).astype(np.int64)
    prob_of = {(int(k), int(i)): p for p, (k, i) in enumerate(zip(ev['prob_cat'], ev['prob_img']))}
    out = dict(ev)
    out['iou_off'] = np.concatenate([[0], np.cumsum(dcount * gcount)]).astype(np.int32)
    out['iou'] = np.zeros(int(out['iou_off'][-1]), np.float64)
    out['dt_box'] = np.zeros((ND, 4), np.int32)
    out['dt_area'] = np.zeros(ND, np.int32)
    out['dt_best'], out['dt_iou'] = np.zeros(ND, np.int32), np.full(ND, -1000.0)
    out['dt_tp'], out['dt_fp'] = np.zeros((T, ND), np.uint8), np.zeros((T, ND), np.uint8)
    out['gt_det'] = np.zeros((T, NG), np.int32)
    out['order'] = np.zeros(ND, np.int32)
    out['rec'], out['prec'] = np.zeros((T, ND)), np.zeros((T, ND))
    out['npos'] = np.zeros(K, np.int32)
    out['ap07'], out['ap_area'] = np.zeros((T, K)), np.zeros((T, K))
    bounds = np.round(np.asarray(gt['bound'], np.float64)).astype(int).reshape(-1, 4)
    masks_gt = [gt_mask(gt, n) for n in range(NG)]
    for k in range(K):
        c0, c1 = int(ev['cls_off'][k]), int(ev['cls_off'][k + 1])
        p0, p1 = int(ev['cat_off'][k]), int(ev['cat_off'][k + 1])
        num_pos = int(ev['gt_off'][p1] - ev['gt_off'][p0])
        out['npos'][k] = num_pos
        nd = c1 - c0
        if defect == 'unstable_ties':
            sorted_inds = np.array(sorted(range(nd), key=lambda r: (-scores[c0 + r], -r)), np.int64)
        else:
            sorted_inds = np.argsort(-scores[c0:c1], kind='stable')          # the reference's sort is not stable: see the module docstring
        out['order'][c0:c1] = c0 + sorted_inds
        cand = []                                     # per detection in sorted order: (row, problem, cur_overlap, cur_overlap_ind)
        for d in range(nd):
            n = c0 + int(sorted_inds[d])
            p = prob_of[k, int(dt['image'][n])]
            gi = ev['gt_perm'][ev['gt_off'][p]:ev['gt_off'][p + 1]]
            pred_box = round_box(raw[n], defect)
            pred_mask = binarise(dt['masks'][n], pred_box, binary_thresh, defect)
            out['dt_box'][n], out['dt_area'][n] = pred_box, int(pred_mask.sum())
            cur, ind = -1000, -1
            for j, g in enumerate(gi):
                ov = mask_overlap(bounds[g], pred_box, masks_gt[g], pred_mask, defect)
                out['iou'][out['iou_off'][p] + (n - ev['dt_off'][p]) * len(gi) + j] = ov
                if ov >= cur if defect == 'last_of_equal' else ov > cur:
                    cur, ind = ov, j
            out['dt_best'][n], out['dt_iou'][n] = ind + 1, cur
            cand.append((n, p, cur, ind))
        for t, ov_thresh in enumerate(thresholds):
            already = {}                                                         # (problem, instance) -> the detection that took it
            tp, fp = np.zeros(nd), np.zeros(nd)
            for d in range(nd):
                n, p, cur, ind = cand[d]
                if ind < 0:                                                      # the image has no instance of the class
                    fp[d] = 1
                    continue
                if cur > ov_thresh if defect == 'strict_threshold' else cur >= ov_thresh:
                    if (p, ind) in already and defect != 'no_already':
                        fp[d] = 1
                    else:
                        tp[d] = 1
                        if (p, ind) not in already:
                            already[p, ind] = n
                            out['gt_det'][t, ev['gt_off'][p] + ind] = n - ev['dt_off'][p] + 1
                else:
                    fp[d] = 1
            out['dt_tp'][t, c0 + sorted_inds] = tp.astype(np.uint8)
            out['dt_fp'][t, c0 + sorted_inds] = fp.astype(np.uint8)
            fp = np.cumsum(fp)
            tp = np.cumsum(tp)
            rec = tp / float(num_pos)
            prec = tp / np.maximum(fp + tp, np.finfo(np.float64).eps)
            out['rec'][t, c0:c1], out['prec'][t, c0:c1] = rec, prec
            out['ap07'][t, k] = voc_ap(rec, prec, True)
            out['ap_area'][t, k] = voc_ap(rec, prec, False)
    return out


def summary(ap, class_names, thresholds=(0.5, 0.7)):
    """the lines of the box evaluation's summary (tests/voc_eval_ref.py::summary) for the 11-point AP voc_eval_sds returns"""
    return box_ref.summary(ap, class_names, True, thresholds)
