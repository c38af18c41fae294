"""Plain-numpy restatement of the reference's proposal roidb code: nmsp (lib/nms/nms.py:48-86), bbox_overlaps_cython
(lib/bbox/bbox.pyx:35-56), and load_rpn_data / create_roidb_from_box_list / merge_roidbs / evaluate_recall of
lib/dataset/imdb.py:81-204, 291-419.  Every float operation in the reference's precision and order; tests/test_prop_roidb_cpu.py
holds it to the reference's own output (tests/golden/proproidb_v1.npz) on the bits.

Two layers: the reference's functions on per-image lists, and the same work on the device's input layout (rows + prefix offsets)
returning every array the device returns (`nms_ref`, `assign_ref`, `recall_ref`).

The one thing defined here and not by the reference: the NMS order of equal scores is `argsort(kind='stable')[::-1]`, the later
row first (the reference's plain argsort is an unstable sort, so its order of equal scores is undefined)."""
import numpy as np

AREA_NAMES = ['all', '0-25', '25-50', '50-100', '100-200', '200-300', '300-inf']
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 25 ** 2], [25 ** 2, 50 ** 2], [50 ** 2, 100 ** 2],
               [100 ** 2, 200 ** 2], [200 ** 2, 300 ** 2], [300 ** 2, 1e5 ** 2]]


def default_thresholds():
    return np.arange(0.5, 0.95 + 1e-5, 0.05)


def bbox_overlaps(boxes, query_boxes):
    """bbox.pyx:35-56 in float64: overlaps[n, k], one rounding per operation, zero where iw <= 0 or ih <= 0"""
    b, q = np.asarray(boxes, np.float64)[:, None, :], np.asarray(query_boxes, np.float64)[None, :, :]
    box_area = (q[..., 2] - q[..., 0] + 1) * (q[..., 3] - q[..., 1] + 1)
    iw = np.minimum(b[..., 2], q[..., 2]) - np.maximum(b[..., 0], q[..., 0]) + 1
    ih = np.minimum(b[..., 3], q[..., 3]) - np.maximum(b[..., 1], q[..., 1]) + 1
    ua = (b[..., 2] - b[..., 0] + 1) * (b[..., 3] - b[..., 1] + 1) + box_area - iw * ih
    with np.errstate(divide='ignore', invalid='ignore'):
        ov = iw * ih / ua
    return np.where((iw > 0) & (ih > 0), ov, 0.0)


def nmsp(dets, thresh=0.7):
    """nms.py:48-86 on (n,5) rows in their own dtype (float32 in the pipeline); a python float threshold compares in the array's
    dtype.  -> keep (list of row indices in keep order)"""
    if dets.shape[0] == 0:
        return []
    x1, y1, x2, y2, scores = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3], dets[:, 4]
    areas = (x2 - x1 + 1) * (y2 - y1 + 1)
    order = scores.argsort(kind='stable')[::-1]
    thresh = dets.dtype.type(thresh)
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        xx1, yy1 = np.maximum(x1[i], x1[order[1:]]), np.maximum(y1[i], y1[order[1:]])
        xx2, yy2 = np.minimum(x2[i], x2[order[1:]]), np.minimum(y2[i], y2[order[1:]])
        w, h = np.maximum(dets.dtype.type(0.0), xx2 - xx1 + 1), np.maximum(dets.dtype.type(0.0), yy2 - yy1 + 1)
        inter = w * h
        ovr = inter / (areas[i] + areas[order[1:]] - inter)
        order = order[np.where(ovr <= thresh)[0] + 1]
    return keep


def greedy_match(overlaps):
    """imdb.py:353-372 on a copy of the (N, G) matrix -> _gt_overlaps (G)"""
    overlaps = overlaps.copy()
    out = np.zeros(overlaps.shape[1])
    for j in range(min(overlaps.shape[0], overlaps.shape[1])):
        argmax_overlaps = overlaps.argmax(axis=0)
        max_overlaps = overlaps.max(axis=0)
        gt_ind = max_overlaps.argmax()
        gt_ovr = max_overlaps.max()
        assert gt_ovr >= 0
        box_ind = argmax_overlaps[gt_ind]
        out[j] = overlaps[box_ind, gt_ind]
        assert out[j] == gt_ovr
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
    return out


# ---- the reference's functions, per-image lists -----------------------------------------------------------------------------------
def load_rpn_data(box_list):
    """imdb.py:98-112 without the files -> the NMS'd rows per image"""
    out = []
    for b in box_list:
        t = np.array(b)
        out.append(t[np.array(nmsp(t), np.int64)])
    return out


def create_roidb_from_box_list(box_list, gt_roidb, num_classes):
    roidb = []
    for i, rec in enumerate(gt_roidb):
        boxes = box_list[i]
        scores, boxes = boxes[:, -1], boxes[:, :4]
        num_boxes = boxes.shape[0]
        overlaps = np.zeros((num_boxes, num_classes), dtype=np.float32)
        if rec['boxes'].size > 0:
            gt_overlaps = bbox_overlaps(boxes.astype(float), rec['boxes'].astype(float))
            argmaxes, maxes = gt_overlaps.argmax(axis=1), gt_overlaps.max(axis=1)
            pos = np.where(maxes > 0)[0]
            overlaps[pos, rec['gt_classes'][argmaxes[pos]]] = maxes[pos]
        roidb.append({'image': rec['image'], 'height': rec['height'], 'width': rec['width'], 'boxes': boxes,
                      'gt_classes': np.zeros((num_boxes,), dtype=np.int32), 'gt_overlaps': overlaps,
                      'max_classes': overlaps.argmax(axis=1), 'max_overlaps': overlaps.max(axis=1), 'flipped': False,
                      'proposal_scores': scores})
    return roidb


def merge_roidbs(a, b):
    """imdb.py:399-419; the last condition looks the key up in the LISTS, so b's scores are never appended"""
    assert len(a) == len(b)
    for i in range(len(a)):
        if 'proposal_scores' not in a[i]:
            a[i]['proposal_scores'] = 10 * np.ones(a[i]['boxes'].shape[0])
        if 'proposal_scores' not in b[i]:
            b[i]['proposal_scores'] = 10 * np.ones(b[i]['boxes'].shape[0])
        a[i]['boxes'] = np.vstack((a[i]['boxes'], b[i]['boxes']))
        a[i]['gt_classes'] = np.hstack((a[i]['gt_classes'], b[i]['gt_classes']))
        if 'gt_overlaps' in a[i] and 'gt_overlaps' in b[i]:
            a[i]['gt_overlaps'] = np.vstack((a[i]['gt_overlaps'], b[i]['gt_overlaps']))
        else:
            a[i].pop('gt_overlaps', None)
        a[i]['max_classes'] = np.hstack((a[i]['max_classes'], b[i]['max_classes']))
        a[i]['max_overlaps'] = np.hstack((a[i]['max_overlaps'], b[i]['max_overlaps']))
        if 'proposal_scores' in a or 'proposal_scores' in b:
            a[i]['proposal_scores'] = np.hstack((a[i]['proposal_scores'], b[i]['proposal_scores']))
    return a


def evaluate_recall(roidb, candidate_boxes=None, thresholds=None, area_names=None, area_ranges=None):
    """imdb.py:291-396 -> dict(summary, area_counts, num_pos, hits, recalls, ar, gt_overlaps)"""
    area_names = AREA_NAMES if area_names is None else area_names
    area_ranges = AREA_RANGES if area_ranges is None else area_ranges
    num_images = len(roidb)
    info = ''

    def boxes_of(i):
        if candidate_boxes is None:
            return roidb[i]['boxes'][np.where(roidb[i]['gt_classes'] == 0)[0], :]
        return candidate_boxes[i]
    area_counts = []
    for area_name, area_range in zip(area_names[1:], area_ranges[1:]):
        area_count = 0
        for i in range(num_images):
            boxes = boxes_of(i)
            boxes_areas = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
            area_count += len(np.where((boxes_areas >= area_range[0]) & (boxes_areas < area_range[1]))[0])
        area_counts.append(area_count)
    total_counts = float(sum(area_counts))
    for area_name, area_count in zip(area_names[1:], area_counts):
        info += 'percentage of {} {}'.format(area_name, area_count / total_counts)
    info += 'average number of proposal {}'.format(total_counts / num_images)
    out = {'area_counts': np.array(area_counts, np.int64), 'num_pos': [], 'hits': [], 'recalls': [], 'ar': [], 'gt_overlaps': []}
    for area_name, area_range in zip(area_names, area_ranges):
        gt_overlaps = np.zeros(0)
        num_pos = 0
        for i in range(num_images):
            rec = roidb[i]
            max_gt_overlaps = rec['gt_overlaps'].max(axis=1) if 'gt_overlaps' in rec else rec['max_overlaps']
            gt_inds = np.where((rec['gt_classes'] > 0) & (max_gt_overlaps == 1))[0]
            gt_boxes = rec['boxes'][gt_inds, :]
            gt_areas = (gt_boxes[:, 2] - gt_boxes[:, 0] + 1) * (gt_boxes[:, 3] - gt_boxes[:, 1] + 1)
            valid_gt_inds = np.where((gt_areas >= area_range[0]) & (gt_areas < area_range[1]))[0]
            gt_boxes = gt_boxes[valid_gt_inds, :]
            num_pos += len(valid_gt_inds)
            boxes = boxes_of(i)
            if boxes.shape[0] == 0:
                continue
            overlaps = bbox_overlaps(boxes[:, :4].astype(float), gt_boxes.astype(float))
            gt_overlaps = np.hstack((gt_overlaps, greedy_match(overlaps)))
        gt_overlaps = np.sort(gt_overlaps)
        if thresholds is None:
            thresholds = default_thresholds()
        recalls = np.zeros_like(thresholds)
        hits = np.zeros(len(thresholds), np.int64)
        with np.errstate(divide='ignore', invalid='ignore'):
            for i, t in enumerate(thresholds):
                hits[i] = (gt_overlaps >= t).sum()
                recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
        ar = recalls.mean()
        info += 'average recall for {}: {:.3f}'.format(area_name, ar)
        for threshold, recall in zip(thresholds, recalls):
            info += 'recall @{:.2f}: {:.3f}'.format(threshold, recall)
        for k, v in (('num_pos', num_pos), ('hits', hits), ('recalls', recalls), ('ar', ar), ('gt_overlaps', gt_overlaps)):
            out[k].append(v)
    out['summary'] = info
    out['num_pos'], out['hits'] = np.array(out['num_pos'], np.int64), np.array(out['hits'], np.int64)
    out['recalls'], out['ar'] = np.array(out['recalls']), np.array(out['ar'])
    return out


# ---- the same work on the device's layout ---------------------------------------------------------------------------------------------
def nms_ref(rows, off, thresh=0.7):
    """rows (total,5) f32, off (I+1) -> keep (total) i32 (per image: the kept indices, then -1), nkeep (I) i32"""
    keep, nkeep = np.full(len(rows), -1, np.int32), np.zeros(len(off) - 1, np.int32)
    for b in range(len(off) - 1):
        k = nmsp(rows[off[b]:off[b + 1]], thresh)
        keep[off[b]:off[b] + len(k)] = k
        nkeep[b] = len(k)
    return {'keep': keep, 'nkeep': nkeep}


def assign_ref(boxes, box_off, gt, gt_classes, gt_off):
    """-> max_ov (total) f32, max_cls (total) i32, argmax (total) i32 (-1 in an image without ground truth)"""
    n = len(boxes)
    out = {'max_ov': np.zeros(n, np.float32), 'max_cls': np.zeros(n, np.int32), 'argmax': np.full(n, -1, np.int32)}
    for i in range(len(box_off) - 1):
        s, g = slice(box_off[i], box_off[i + 1]), slice(gt_off[i], gt_off[i + 1])
        if gt_off[i + 1] == gt_off[i] or box_off[i + 1] == box_off[i]:
            continue
        ov = bbox_overlaps(boxes[s], gt[g])
        argmaxes, maxes = ov.argmax(axis=1), ov.max(axis=1)
        out['max_ov'][s] = maxes                                   # the assignment into a float32 array
        out['max_cls'][s] = np.where(maxes > 0, gt_classes[g][argmaxes], 0)
        out['argmax'][s] = argmaxes
    return out


def recall_ref(boxes, box_off, gt, gt_mask, gt_off, A, thresholds):
    """-> gt_ov (A,NG) f64 (per image and range: the G_a values of _gt_overlaps, then zeros up to the image's G rows), num_pos (A)
    i32, hits (A,T) i32"""
    thrs = np.asarray(thresholds, np.float64)
    NG = len(gt)
    out = {'gt_ov': np.zeros((A, NG)), 'num_pos': np.zeros(A, np.int32), 'hits': np.zeros((A, len(thrs)), np.int32)}
    for a in range(A):
        for i in range(len(box_off) - 1):
            g0 = gt_off[i]
            sel = g0 + np.flatnonzero((gt_mask[g0:gt_off[i + 1]] >> a) & 1)
            out['num_pos'][a] += len(sel)
            b = boxes[box_off[i]:box_off[i + 1]]
            if len(b) == 0:
                continue
            vals = greedy_match(bbox_overlaps(b, gt[sel]))
            out['gt_ov'][a, g0:g0 + len(sel)] = vals
            out['hits'][a] += (vals[None, :] >= thrs[:, None]).sum(axis=1).astype(np.int32)
    return out
