"""COCO box evaluation on the device: the last line of the reference's test run, `imdb.evaluate_detections(all_boxes)`
(lib/inference.py:523-527 -> lib/dataset/coco.py -> lib/dataset/pycocotools/cocoeval.py).

    result = evaluate_detections(all_boxes, roidb, num_classes)      # all_boxes as Tester.aggregate returns it
    print(result.summary())

The per-image matching and the accumulation run as sn_coco_match / sn_coco_accumulate (sniper_amd/csrc/coco_eval.hip, DESIGN.md
section 19): float64 IoU, integer counts, a few float64 divisions -- `precision` and `recall` are the reference's arrays on their
bits.  The host's share is the conversion of the detections into the reference's result rows (coco.py:36-48 and COCO.loadRes),
the CSR offsets of the (category, image) problems (numpy, vectorised) and the twelve means of summarize().  There is no CPU
fallback: without the kernel library or a GPU, evaluate() raises.

The reference's second data set, PASCAL VOC, ends in the same line through voc_eval / voc_ap: evaluate_detections_voc and
VOCBoxEvaluator in the second half of this file (sn_voc_match / sn_voc_accumulate, sniper_amd/csrc/voc_eval.hip, DESIGN.md
section 20).

COCO masks (`imdb.evaluate_sds`, COCOeval with useSegm = 1) from run-length encoded masks: COCOSegmEvaluator at the end of this
file (sn_rle_stats / sn_rle_iou / sn_coco_match_iou, sniper_amd/csrc/coco_segm.hip).

PASCAL VOC masks (voc_eval_sds, the mask AP of the FCIS / DCN lineage): evaluate_sds_voc and VOCSegmEvaluator, last in this file
(sn_vocsds_mask_iou / sn_vocsds_match_iou, sniper_amd/csrc/voc_segm.hip).
"""
import numpy as np

__all__ = ['Params', 'COCOBoxEvaluator', 'COCOBoxResult', 'evaluate_detections', 'round_half_even_decimal']


class Params(object):
    """The reference's Params (cocoeval.py:436-445).  useSegm belongs to COCOSegmEvaluator (COCOBoxEvaluator refuses it); useCats = 0
    is not implemented."""

    def __init__(self):
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.useSegm = 0
        self.useCats = 1


def round_half_even_decimal(x, ndigits):
    """Python's round(float(v), ndigits) for every v of a float64 array (the reference rounds with the builtin: correctly rounded in
    decimal, which np.round -- rint(v * 10**n) / 10**n -- misses where v * 10**n lands on the other side of a half).  Vectorised:
    rint(v * 10**n) / 10**n is the builtin's answer whenever v * 10**n is not within 1e-6 of a half (the quotient k / 10**n is the
    double nearest to that decimal either way); the few values that are go through the builtin."""
    x = np.asarray(x, np.float64)
    s = float(10 ** ndigits)
    y = x * s
    out = np.rint(y) / s
    near = np.abs(np.abs(y - np.floor(y)) - 0.5) < 1e-6
    near |= ~(np.abs(y) < 2.0 ** 51)              # huge, inf, nan: leave them to the builtin too
    if near.any():
        flat, idx = out.reshape(-1), np.flatnonzero(near.reshape(-1))
        src = x.reshape(-1)
        flat[idx] = [round(float(src[i]), ndigits) for i in idx]
        out = flat.reshape(x.shape)
    return out


_STAT_ROWS = ((1, None, 'all', 100), (1, .5, 'all', 100), (1, .75, 'all', 100), (1, None, 'small', 100), (1, None, 'medium', 100),
              (1, None, 'large', 100), (0, None, 'all', 1), (0, None, 'all', 10), (0, None, 'all', 100), (0, None, 'small', 100),
              (0, None, 'medium', 100), (0, None, 'large', 100))


class COCOBoxResult(object):
    """precision (T,R,K,A,M), recall (T,K,A,M), stats (12,), per_class_ap (K,), summary()"""

    def __init__(self, precision, recall, params, cat_ids, timing=None):
        self.precision, self.recall, self.params, self.cat_ids = precision, recall, params, list(cat_ids)
        self.timing = timing or {}
        self.stats, self._lines = self._summarize()
        self.per_class_ap, self.mean_ap = self._per_class()

    def _summarize(self):
        """cocoeval.py:376-427: like the reference it addresses the default area ranges and maxDets by position"""
        p = self.params
        stats, lines = np.zeros((12,)), []
        for n, (ap, iou_thr, area, max_dets) in enumerate(_STAT_ROWS):
            aind = [i for i, name in enumerate(['all', 'small', 'medium', 'large']) if name == area]
            mind = [i for i, md in enumerate([1, 10, 100]) if md == max_dets]
            if aind[0] >= self.recall.shape[2] or mind[0] >= self.recall.shape[3]:
                mean_s = -1                           # custom params with fewer ranges: the row does not exist
            else:
                if ap == 1:
                    s = self.precision
                    if iou_thr is not None:
                        s = s[np.where(iou_thr == p.iouThrs)[0]]
                    s = s[:, :, :, aind, mind]
                else:
                    s = self.recall[:, :, aind, mind]
                mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
            stats[n] = mean_s
            lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6} | maxDets={:>3} ] = {}'.format(
                'Average Precision' if ap == 1 else 'Average Recall', '(AP)' if ap == 1 else '(AR)',
                '%0.2f:%0.2f' % (p.iouThrs[0], p.iouThrs[-1]) if iou_thr is None else '%0.2f' % iou_thr, area, '%d' % max_dets,
                '%.3f' % float(mean_s)))
        return stats, lines

    def _per_class(self):
        """coco.py:338-370: AP over IoU 0.50:0.95, area range 0, the last maxDets, per category (nan where a category has no entry
        above -1, as np.mean of nothing is)"""
        p = self.params

        def thr_ind(thr):
            hit = np.where((p.iouThrs > thr - 1e-5) & (p.iouThrs < thr + 1e-5))[0]
            return int(hit[0]) if len(hit) else None
        lo, hi = thr_ind(0.5), thr_ind(0.95)
        K = self.precision.shape[2]
        if lo is None or hi is None:
            return np.full((K,), np.nan), float('nan')
        pr = self.precision[lo:hi + 1, :, :, 0, self.precision.shape[4] - 1]
        mean_of = lambda v: float(np.mean(v[v > -1])) if (v > -1).any() else float('nan')
        return np.array([mean_of(pr[:, :, k]) for k in range(K)]), mean_of(pr)

    def summary(self):
        """the twelve lines of COCOeval.summarize()"""
        return '\n'.join(self._lines)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    assert off[-1] < 2 ** 31
    return off.astype(np.int32)


def _cell_counts(all_boxes, K, I):
    """(K, I) row counts of all_boxes[class][image] (class 0 = background), its shape checked (both evaluators)"""
    assert len(all_boxes) == K + 1, 'all_boxes[class][image]: %d classes (with the background) for %d categories' % (len(all_boxes), K)
    counts = np.zeros((K, I), np.int64)
    for k in range(K):
        assert len(all_boxes[k + 1]) == I, 'all_boxes[%d] has %d images, the ground truth %d' % (k + 1, len(all_boxes[k + 1]), I)
        counts[k] = np.fromiter(map(len, all_boxes[k + 1]), np.int64, I)
    return counts


def _problem_offsets(dt_counts, gt_category, gt_image):
    """CSR offsets of the (category, image) pairs that have a detection or a box, category-major then by image (both evaluators)"""
    K, I = dt_counts.shape
    gkey = gt_category * I + gt_image
    gt_counts = np.bincount(gkey, minlength=K * I).reshape(K, I)
    has = ((dt_counts + gt_counts) > 0).reshape(-1)
    dc, gc = dt_counts.reshape(-1)[has], gt_counts.reshape(-1)[has]
    prob_cat = np.flatnonzero(has) // I
    return {
        'P': int(has.sum()), 'dt_off': _offsets(dc), 'gt_off': _offsets(gc), 'dt_counts': dc,
        'cat_off': np.searchsorted(prob_cat, np.arange(K + 1)).astype(np.int32),
        'gt_order': np.argsort(gkey, kind='stable'),          # boxes grouped by problem, annotation order inside
        'max_dt': int(dc.max()) if len(dc) else 0, 'max_gt': int(gc.max()) if len(gc) else 0,
    }


class COCOBoxEvaluator(object):
    """gt: dict of arrays over the NG ground-truth boxes in annotation order -- image (index into image_ids), category (index into
    cat_ids), bbox (NG,4) xywh, area, iscrowd, ignore (optional, 0).  params: a Params (default: the reference's)."""

    def __init__(self, gt, image_ids, cat_ids, params=None):
        self.params = params or Params()
        if getattr(self.params, 'useSegm', 0):
            raise NotImplementedError('COCOBoxEvaluator: useSegm (mask evaluation) is not implemented, boxes only')
        if not getattr(self.params, 'useCats', 1):
            raise NotImplementedError('COCOBoxEvaluator: useCats = 0 (category-agnostic evaluation) is not implemented')
        self.image_ids, self.cat_ids = list(image_ids), list(cat_ids)
        n = len(gt['image'])
        self.gt = {
            'image': np.asarray(gt['image'], np.int64).reshape(n), 'category': np.asarray(gt['category'], np.int64).reshape(n),
            'bbox': np.asarray(gt['bbox'], np.float64).reshape(n, 4), 'area': np.asarray(gt['area'], np.float64).reshape(n),
            'iscrowd': np.asarray(gt['iscrowd']).reshape(n).astype(np.int64) != 0,
            'ignore': (np.asarray(gt['ignore']).reshape(n).astype(np.int64) != 0) if 'ignore' in gt else np.zeros(n, bool),
        }
        I, K = len(self.image_ids), len(self.cat_ids)
        assert n == 0 or (0 <= self.gt['image'].min() and self.gt['image'].max() < I), 'gt image index out of range'
        assert n == 0 or (0 <= self.gt['category'].min() and self.gt['category'].max() < K), 'gt category index out of range'

    @classmethod
    def from_roidb(cls, roidb, num_classes, params=None):
        """Ground truth = the roidb rows with gt_classes > 0; xywh = x1, y1, x2-x1+1, y2-y1+1 (float64); area = roidb['gt_areas']
        where present, else w*h; iscrowd = roidb['gt_iscrowd'] where present, else 0.  Image ids are 1.., category ids 1..num_classes-1
        (class c is category index c-1), annotation ids follow the roidb order."""
        img, cat, box, area, crowd = [], [], [], [], []
        for i, r in enumerate(roidb):
            classes = np.asarray(r['gt_classes'])
            keep = np.flatnonzero(classes > 0)
            b = np.asarray(r['boxes'], np.float64)[keep].reshape(-1, 4)
            xywh = np.stack((b[:, 0], b[:, 1], b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1), axis=1)
            img.append(np.full(len(keep), i, np.int64))
            cat.append(classes[keep].astype(np.int64) - 1)
            box.append(xywh)
            area.append(np.asarray(r['gt_areas'], np.float64)[keep] if 'gt_areas' in r else xywh[:, 2] * xywh[:, 3])
            crowd.append(np.asarray(r['gt_iscrowd'])[keep].astype(np.int64) if 'gt_iscrowd' in r else np.zeros(len(keep), np.int64))
        cat0 = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
        gt = {'image': cat0(img, (0,), np.int64), 'category': cat0(cat, (0,), np.int64), 'bbox': cat0(box, (0, 4), np.float64),
              'area': cat0(area, (0,), np.float64), 'iscrowd': cat0(crowd, (0,), np.int64)}
        return cls(gt, range(1, len(roidb) + 1), range(1, num_classes), params)

    # ---- detections -----------------------------------------------------------------------------
    def _counts(self, all_boxes):
        return _cell_counts(all_boxes, len(self.cat_ids), len(self.image_ids))

    def convert_detections(self, all_boxes):
        """coco.py:36-48 + COCO.loadRes (pycocotools/coco.py:305-314) -> (dt rows (ND,6) float64 = x, y, w, h, score, area in
        class-major, image, row order -- the order of the reference's result list, hence of its annotation ids -- and the (K, I)
        row counts): float64 x2-x1+1, box values rounded to 1 decimal and the score to 8 like the builtin round does, area =
        rounded w * rounded h."""
        counts = self._counts(all_boxes)
        cells = [d for per_image in all_boxes[1:] for d in per_image if len(d)]
        rows = np.concatenate(cells, axis=0).astype(np.float64).reshape(-1, 5) if cells else np.zeros((0, 5), np.float64)
        dt = np.empty((len(rows), 6), np.float64)
        dt[:, 0], dt[:, 1] = rows[:, 0], rows[:, 1]
        dt[:, 2] = rows[:, 2] - rows[:, 0] + 1
        dt[:, 3] = rows[:, 3] - rows[:, 1] + 1
        dt[:, :4] = round_half_even_decimal(dt[:, :4], 1)
        dt[:, 4] = round_half_even_decimal(rows[:, 4], 8)
        dt[:, 5] = dt[:, 2] * dt[:, 3]
        return dt, counts

    def _device_rows(self, all_boxes):
        """round_results=False: the cells' rows stacked on the device (torch.cat of device cells = copies in HBM; host cells are stacked
        and uploaded once) -> ((ND,5) device tensor float32 or float64, (K, I) counts)"""
        import torch
        from . import hip
        counts = self._counts(all_boxes)
        cells = [d for per_image in all_boxes[1:] for d in per_image if len(d)]
        if not cells:
            return torch.zeros((0, 5), dtype=torch.float64, device=hip.require_gpu()), counts
        if all(isinstance(d, torch.Tensor) and d.is_cuda for d in cells):
            assert len(set(d.dtype for d in cells)) == 1 and cells[0].dtype in (torch.float32, torch.float64)
            return torch.cat([d.reshape(-1, 5) for d in cells]).contiguous(), counts
        host = [d.cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d) for d in cells]
        dtype = np.float32 if all(h.dtype == np.float32 for h in host) else np.float64
        return hip.dev(np.concatenate([h.reshape(-1, 5).astype(dtype, copy=False) for h in host])), counts

    # ---- the problems ---------------------------------------------------------------------------
    def _problems(self, dt_counts, max_det):
        """CSR offsets of the (category, image) pairs that have a detection or a box, category-major then by image"""
        pr = _problem_offsets(dt_counts, self.gt['category'], self.gt['image'])
        pr['kp_off'] = _offsets(np.minimum(pr.pop('dt_counts'), max_det))
        return pr

    def evaluate(self, all_boxes, round_results=True, return_matches=False):
        """all_boxes[class][image] = (n,5) rows x1, y1, x2, y2, score (class 0 = background) -> COCOBoxResult.
        round_results=False skips the reference's rounding of the result rows (1 decimal for boxes, 8 for scores) and takes device-
        resident rows (CUDA tensors in the cells) without a host copy: the numbers are then those of the unrounded detections, NOT the
        reference's.  return_matches adds the per-image arrays (sn_coco_match's outputs and the offsets) as result.matches."""
        import torch
        from . import hip
        p = self.params
        dev = hip.require_gpu()
        iou_thrs, rec_thrs = np.asarray(p.iouThrs, np.float64), np.asarray(p.recThrs, np.float64)
        area_rng = np.asarray(p.areaRng, np.float64).reshape(-1, 2)
        max_dets = np.asarray(sorted(p.maxDets), np.int32)
        T, R, A, M, K = len(iou_thrs), len(rec_thrs), len(area_rng), len(max_dets), len(self.cat_ids)
        max_det = int(max_dets[-1])
        t0 = _now(torch)
        rows = None
        if round_results:
            dt_host, counts = self.convert_detections(all_boxes)
            ND = len(dt_host)
        else:
            rows, counts = self._device_rows(all_boxes)
            ND = len(rows)
        pr = self._problems(counts, max_det)
        P, NG = pr['P'], len(self.gt['image'])
        if P == 0:                                    # nothing to evaluate: every category is absent
            return COCOBoxResult(-np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), p, self.cat_ids)
        NK = int(pr['kp_off'][-1])
        o = pr['gt_order']
        gt_rows = np.concatenate((self.gt['bbox'][o], self.gt['area'][o, None]), axis=1) if NG else np.zeros((1, 5))
        flags = (self.gt['iscrowd'][o].astype(np.uint8) | (self.gt['ignore'][o].astype(np.uint8) << 1)) if NG else np.zeros(1, np.uint8)
        kept_per_cat = np.diff(pr['kp_off'][pr['cat_off']].astype(np.int64))
        t1 = _now(torch)
        if rows is None:
            d_dt = hip.dev(dt_host) if ND else torch.zeros((1, 6), dtype=torch.float64, device=dev)
        else:
            d_dt = torch.empty((max(ND, 1), 6), dtype=torch.float64, device=dev)
            if ND:
                hip.call('sn_coco_pack_rows', rows, int(rows.dtype == torch.float32), None, ND, d_dt, hip.stream())
        d_gt, d_flags = hip.dev(gt_rows), hip.dev(flags)
        d_dt_off, d_gt_off, d_kp_off, d_cat_off = (hip.dev(pr[k]) for k in ('dt_off', 'gt_off', 'kp_off', 'cat_off'))
        d_iou, d_rec, d_area = hip.dev(iou_thrs), hip.dev(rec_thrs), hip.dev(area_rng)
        i32 = lambda *shape: torch.empty([max(int(np.prod(shape)), 1)], dtype=torch.int32, device=dev)
        u8 = lambda *shape: torch.empty([max(int(np.prod(shape)), 1)], dtype=torch.uint8, device=dev)
        dt_rank, dt_match, dt_ignore = i32(NK), i32(A, T, NK), u8(A, T, NK)
        gt_match, gt_ignore = i32(A, T, NG), u8(A, NG)
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        ws = torch.empty(int(hip.query('sn_coco_accumulate_workspace_bytes', NK, T, A)), dtype=torch.uint8, device=dev)
        t2 = _now(torch)
        hip.call('sn_coco_match', d_dt, d_dt_off, d_kp_off, d_gt, d_flags, d_gt_off, d_iou, d_area, P, T, A, max_det, pr['max_dt'],
                 pr['max_gt'], NK, NG, dt_rank, dt_match, dt_ignore, gt_match, gt_ignore, hip.stream())
        tm = _now(torch)
        hip.call('sn_coco_accumulate', d_dt, d_dt_off, d_kp_off, d_gt_off, d_cat_off, dt_rank, dt_match, dt_ignore, gt_ignore, d_rec,
                 max_dets, P, K, T, A, M, R, max_det, int(kept_per_cat.max()), NK, NG, ws, ws.numel(), precision, recall, hip.stream())
        t3 = _now(torch)
        h_precision, h_recall = precision.cpu().numpy(), recall.cpu().numpy()
        t4 = _now(torch)
        # seconds: host = result rows + CSR offsets, upload = allocations + copies to the device, kernels = sn_coco_match +
        # sn_coco_accumulate, download = precision + recall to the host
        res = COCOBoxResult(h_precision, h_recall, p, self.cat_ids,
                            {'host_s': t1 - t0, 'upload_s': t2 - t1, 'kernels_s': t3 - t2, 'match_s': tm - t2, 'accumulate_s': t3 - tm, 'download_s': t4 - t3, 'problems': P,
                             'detections': ND, 'kept': NK, 'boxes': NG})
        if return_matches:
            res.matches = dict(pr, NK=NK, dt_rank=dt_rank[:NK].cpu().numpy(), dt_match=dt_match[:A * T * NK].reshape(A, T, NK).cpu().numpy(),
                               dt_ignore=dt_ignore[:A * T * NK].reshape(A, T, NK).cpu().numpy(),
                               gt_match=gt_match[:A * T * NG].reshape(A, T, NG).cpu().numpy(),
                               gt_ignore=gt_ignore[:A * NG].reshape(A, NG).cpu().numpy(), dt=d_dt[:ND].cpu().numpy())
        return res


def _now(torch):
    import time
    torch.cuda.synchronize()
    return time.perf_counter()


def evaluate_detections(all_boxes, roidb, num_classes, params=None, round_results=True):
    """`imdb.evaluate_detections(all_boxes)` of the reference's test run in one call: ground truth from the roidb, detections as
    Tester.aggregate / imdb_detection_wrapper return them -> COCOBoxResult"""
    return COCOBoxEvaluator.from_roidb(roidb, num_classes, params).evaluate(all_boxes, round_results=round_results)


# ---- PASCAL VOC --------------------------------------------------------------------------------------
# The reference's second data set (configs/faster/sniper_res101_e2e_pascal_voc.yml) ends in the same line through
# PascalVOC.evaluate_detections -> write_pascal_results -> do_python_eval -> voc_eval / voc_ap (lib/dataset/pascal_voc.py:246-265,
# 395-456, lib/dataset/pascal_voc_eval.py:39-181).  sn_voc_match / sn_voc_accumulate (sniper_amd/csrc/voc_eval.hip, DESIGN.md
# section 20) do the matching and the curves; the host converts the detections into the rows of the result files and takes the means.
#
# EQUAL SCORES.  Rounding scores to 3 decimals makes equal scores common, and the reference's np.argsort(-confidence) is not a
# stable sort, so the reference itself does not define their order.  This project does: arrival order = class-major, image, row.
VOC_CLASSES = ('aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog', 'horse',
               'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor')

__all__ += ['VOCBoxEvaluator', 'VOCBoxResult', 'evaluate_detections_voc', 'VOC_CLASSES']


class VOCBoxResult(object):
    """ap07, ap_area (T,K); ap = the one `use_07_metric` chooses; mean_ap (T,); npos (K,); summary()"""

    def __init__(self, ap07, ap_area, npos, class_names, use_07_metric, thresholds, timing=None):
        self.ap07, self.ap_area, self.npos = ap07, ap_area, npos
        self.class_names, self.use_07_metric, self.thresholds = list(class_names), bool(use_07_metric), tuple(thresholds)
        self.ap = ap07 if use_07_metric else ap_area
        self.mean_ap = np.array([np.mean(self.ap[t]) for t in range(len(self.thresholds))], np.float64)
        self.timing = timing or {}

    def summary(self):
        """the info_str of do_python_eval (pascal_voc.py:417-456), character for character"""
        blocks = []
        for t, thr in enumerate(self.thresholds):
            lines = ['AP for {} = {:.4f}'.format(c, self.ap[t, k]) for k, c in enumerate(self.class_names)]
            lines.append('Mean AP@{:g} = {:.4f}'.format(thr, self.mean_ap[t]))
            blocks.append('\n'.join(lines))
        return 'VOC07 metric? ' + ('Y' if self.use_07_metric else 'No') + '\n' + '\n\n'.join(blocks)

    def curve(self, t, k):
        """(rec, prec) of class k at threshold t (evaluate(..., return_curves=True) only)"""
        lo, hi = self.curves['cls_off'][k], self.curves['cls_off'][k + 1]
        return self.curves['rec'][t, lo:hi], self.curves['prec'][t, lo:hi]


class VOCBoxEvaluator(object):
    """gt: dict of arrays over the NG annotated boxes in annotation order -- image (index, 0 .. num_images - 1), category (index
    into class_names), bbox (NG,4) x1, y1, x2, y2 AS THE ANNOTATION HOLDS THEM (1-based like the XML), difficult.  class_names: the K
    foreground classes (a leading '__background__' is dropped).  use_07_metric: the 11-point AP (True) or the area under the
    monotone envelope (False) as `ap`; both are computed on every call."""

    def __init__(self, gt, num_images, class_names, use_07_metric, thresholds=(0.5, 0.7)):
        names = list(class_names)
        self.class_names = names[1:] if names and names[0] == '__background__' else names
        self.num_images, self.use_07_metric = int(num_images), bool(use_07_metric)
        self.thresholds = tuple(float(t) for t in thresholds)
        n = len(gt['image'])
        self.gt = {
            'image': np.asarray(gt['image'], np.int64).reshape(n), 'category': np.asarray(gt['category'], np.int64).reshape(n),
            'bbox': np.asarray(gt['bbox'], np.float64).reshape(n, 4),
            'difficult': (np.asarray(gt['difficult']).reshape(n).astype(np.int64) != 0) if 'difficult' in gt else np.zeros(n, bool),
        }
        K = len(self.class_names)
        assert n == 0 or (0 <= self.gt['image'].min() and self.gt['image'].max() < self.num_images), 'gt image index out of range'
        assert n == 0 or (0 <= self.gt['category'].min() and self.gt['category'].max() < K), 'gt category index out of range'

    @classmethod
    def from_roidb(cls, roidb, num_classes, class_names=None, year='2007'):
        """Ground truth = the roidb rows with gt_classes > 0; boxes = roidb['boxes'] + 1 (the loader subtracted 1 from the XML's
        pixel indices, pascal_voc.py:170-173); difficult = roidb[i]['gt_difficult'] where present, else all zero; use_07_metric by
        the reference's rule, year == 'SDS' or int(year) < 2010.

        NOTE: the reference's own roidb DROPS difficult objects (use_diff: False) while voc_eval reads them from the XML, where
        they shield the detections that match them from counting as false positives.  A caller who wants the reference's numbers
        on real VOC must keep those objects in the roidb and pass their flags as 'gt_difficult'."""
        if class_names is None:
            class_names = VOC_CLASSES if num_classes == len(VOC_CLASSES) + 1 else ['class%d' % c for c in range(1, num_classes)]
        names = list(class_names)
        names = names[1:] if names and names[0] == '__background__' else names
        assert len(names) == num_classes - 1, '%d class names for %d classes with the background' % (len(names), num_classes)
        img, cat, box, diff = [], [], [], []
        for i, r in enumerate(roidb):
            classes = np.asarray(r['gt_classes'])
            keep = np.flatnonzero(classes > 0)
            img.append(np.full(len(keep), i, np.int64))
            cat.append(classes[keep].astype(np.int64) - 1)
            box.append(np.asarray(r['boxes'], np.float64)[keep].reshape(-1, 4) + 1)
            diff.append(np.asarray(r['gt_difficult'])[keep].astype(np.int64) if 'gt_difficult' in r else np.zeros(len(keep), np.int64))
        cat0 = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)
        gt = {'image': cat0(img, (0,), np.int64), 'category': cat0(cat, (0,), np.int64), 'bbox': cat0(box, (0, 4), np.float64),
              'difficult': cat0(diff, (0,), np.int64)}
        return cls(gt, len(roidb), names, year == 'SDS' or int(year) < 2010)

    def convert_detections(self, all_boxes):
        """The rows write_pascal_results writes ('{:.3f}' of the score, '{:.1f}' of v + 1, pascal_voc.py:412-415) and voc_eval reads
        back -> ((ND,5) float64 rows x1, y1, x2, y2, score in class-major, image, row order, (K, I) row counts).  v + 1 is taken in
        the rows' own dtype (float32 rows add in float32, as dets[k, 0] + 1 does), then converted to float64 and rounded like the
        format does: correctly in decimal, halves to even."""
        counts = _cell_counts(all_boxes, len(self.class_names), self.num_images)
        cells = [d for per_image in all_boxes[1:] for d in per_image if len(d)]
        cells = [np.asarray(d.cpu() if hasattr(d, 'cpu') else d).reshape(-1, 5) for d in cells]
        if not cells:
            return np.zeros((0, 5), np.float64), counts
        if len(set(c.dtype for c in cells)) == 1:
            raw = np.concatenate(cells, axis=0)
            plus = (raw[:, :4] + 1).astype(np.float64)
            score = raw[:, 4].astype(np.float64)
        else:
            plus = np.concatenate([(c[:, :4] + 1).astype(np.float64) for c in cells], axis=0)
            score = np.concatenate([c[:, 4].astype(np.float64) for c in cells], axis=0)
        rows = np.empty((len(plus), 5), np.float64)
        rows[:, :4] = round_half_even_decimal(plus, 1)
        rows[:, 4] = round_half_even_decimal(score, 3)
        return rows, counts

    def evaluate(self, all_boxes, return_curves=False):
        """all_boxes[class][image] = (n,5) rows x1, y1, x2, y2, score, 0-based pixel indices as the test run holds them (class 0 =
        background) -> VOCBoxResult.  return_curves adds result.curves: rec and prec (T,ND) in each class's sorted order, order,
        cls_off (K+1) (class k's curve is [cls_off[k], cls_off[k+1]), result.curve(t, k)), the outputs of sn_voc_match (dt_best,
        dt_iou, dt_tp, dt_fp, gt_det), the rows and the offsets."""
        import torch
        from . import hip
        dev = hip.require_gpu()
        thrs = np.asarray(self.thresholds, np.float64)
        T, K = len(thrs), len(self.class_names)
        t0 = _now(torch)
        rows, counts = self.convert_detections(all_boxes)
        ND, NG = len(rows), len(self.gt['image'])
        pr = _problem_offsets(counts, self.gt['category'], self.gt['image'])
        P = pr['P']
        if P == 0:                                    # neither detections nor boxes: every AP is 0, as the reference's
            return VOCBoxResult(np.zeros((T, K)), np.zeros((T, K)), np.zeros(K, np.int32), self.class_names, self.use_07_metric, self.thresholds)
        o = pr['gt_order']
        gt_rows = self.gt['bbox'][o] if NG else np.zeros((1, 4))
        difficult = self.gt['difficult'][o].astype(np.uint8) if NG else np.zeros(1, np.uint8)
        cls_off = pr['dt_off'][pr['cat_off']]
        per_class = np.diff(cls_off.astype(np.int64))
        ap07_thrs = np.arange(0., 1.1, 0.1)
        assert ap07_thrs.shape == (11,) and ap07_thrs.dtype == np.float64
        t1 = _now(torch)
        d_box = hip.dev(np.ascontiguousarray(rows[:, :4])) if ND else torch.zeros((1, 4), dtype=torch.float64, device=dev)
        d_score = hip.dev(np.ascontiguousarray(rows[:, 4])) if ND else torch.zeros((1,), dtype=torch.float64, device=dev)
        d_gt, d_diff = hip.dev(gt_rows), hip.dev(difficult)
        d_dt_off, d_gt_off, d_cat_off, d_thr = hip.dev(pr['dt_off']), hip.dev(pr['gt_off']), hip.dev(pr['cat_off']), hip.dev(thrs)
        empty = lambda dtype, *shape: torch.empty([max(int(np.prod(shape)), 1)], dtype=dtype, device=dev)
        dt_best, dt_iou = empty(torch.int32, ND), empty(torch.float64, ND)
        dt_tp, dt_fp, gt_det = empty(torch.uint8, T, ND), empty(torch.uint8, T, ND), empty(torch.int32, T, NG)
        order, rec, prec = empty(torch.int32, ND), empty(torch.float64, T, ND), empty(torch.float64, T, ND)
        npos = torch.empty((K,), dtype=torch.int32, device=dev)
        ap07 = torch.empty((T, K), dtype=torch.float64, device=dev)
        ap_area = torch.empty((T, K), dtype=torch.float64, device=dev)
        ws = torch.empty(int(hip.query('sn_voc_accumulate_workspace_bytes', ND, T)), dtype=torch.uint8, device=dev)
        t2 = _now(torch)
        hip.call('sn_voc_match', d_box, d_score, d_dt_off, d_gt, d_diff, d_gt_off, d_thr, P, T, pr['max_dt'], pr['max_gt'], ND, NG,
                 dt_best, dt_iou, dt_tp, dt_fp, gt_det, hip.stream())
        tm = _now(torch)
        hip.call('sn_voc_accumulate', d_score, d_dt_off, d_gt_off, d_cat_off, d_diff, dt_tp, dt_fp, ap07_thrs, P, K, T,
                 int(per_class.max()), ND, NG, ws, ws.numel(), order, rec, prec, npos, ap07, ap_area, hip.stream())
        t3 = _now(torch)
        h_ap07, h_area, h_npos = ap07.cpu().numpy(), ap_area.cpu().numpy(), npos.cpu().numpy()
        curves = None
        if return_curves:
            rd = lambda x, *shape: x[:int(np.prod(shape))].reshape(shape).cpu().numpy()
            curves = dict(pr, cls_off=cls_off, rows=rows, rec=rd(rec, T, ND), prec=rd(prec, T, ND), order=rd(order, ND),
                          dt_best=rd(dt_best, ND), dt_iou=rd(dt_iou, ND), dt_tp=rd(dt_tp, T, ND), dt_fp=rd(dt_fp, T, ND),
                          gt_det=rd(gt_det, T, NG))
        t4 = _now(torch)
        # seconds, the keys of the COCO result: host = result rows + CSR offsets, upload = allocations + copies to the device,
        # kernels = sn_voc_match + sn_voc_accumulate, download = the APs and npos (and the curves, if asked for) to the host
        res = VOCBoxResult(h_ap07, h_area, h_npos, self.class_names, self.use_07_metric, self.thresholds,
                           {'host_s': t1 - t0, 'upload_s': t2 - t1, 'kernels_s': t3 - t2, 'match_s': tm - t2, 'accumulate_s': t3 - tm,
                            'download_s': t4 - t3, 'problems': P, 'detections': ND, 'kept': ND, 'boxes': NG})
        if curves is not None:
            res.curves = curves
        return res


def evaluate_detections_voc(all_boxes, roidb, num_classes, class_names=None, year='2007'):
    """`imdb.evaluate_detections(all_boxes)` of the reference's PASCAL VOC test run in one call: ground truth from the roidb (see
    VOCBoxEvaluator.from_roidb on difficult objects), detections as Tester.aggregate / imdb_detection_wrapper return them ->
    VOCBoxResult; print(result.summary()) gives the reference's lines"""
    return VOCBoxEvaluator.from_roidb(roidb, num_classes, class_names, year).evaluate(all_boxes)


# ---- COCO masks ----------------------------------------------------------------------------------------
# The reference ends a mask run in imdb.evaluate_sds(all_boxes, all_masks) (lib/dataset/coco.py:264-336): COCOeval with useSegm = 1
# over run-length encoded masks, the arithmetic of lib/dataset/pycocotools/maskApi.c.  sn_rle_stats (rleArea, rleToBbox), sn_rle_iou
# (rleIou behind its bounding-box gate) and sn_coco_match_iou do the per-image part, sn_coco_accumulate the curves, unchanged
# (sniper_amd/csrc/coco_segm.hip).  The host decodes string counts, builds the pools and the offsets, and cuts
# the problems into chunks of bounded device memory.
__all__ += ['COCOSegmEvaluator', 'COCOSegmResult', 'evaluate_sds', 'rle_from_string', 'rle_counts', 'rle_from_polys', 'rle_paste', 'paste_boxes']


def rle_from_string(s):
    """rleFrString (maskApi.c:195-208): compressed string counts -> uint32 counts.  Six bits per character from chr(48): five of
    payload, 0x20 = another character follows, 0x10 of the last one = the sign; from the third count on the value is a difference
    to the count two before."""
    if isinstance(s, bytes):
        s = s.decode('ascii')
    cnts, p, n = [], 0, len(s)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError('rle_from_string: the string ends inside a count')
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xFFFFFFFF)
    return np.array(cnts, np.uint32)


def rle_counts(seg, h, w, what):
    """one RLE `segmentation` entry -> its uint32 counts: {'size': [h, w], 'counts': list | array (uncompressed) | str (compressed)}.
    ValueError, naming `what`, where the size is not the image's or the counts do not sum to h * w."""
    if not isinstance(seg, dict) or 'counts' not in seg:
        raise ValueError('%s: a run-length encoded mask is a dict with `size` and `counts`, got %s' % (what, type(seg).__name__))
    if 'size' in seg and (int(seg['size'][0]), int(seg['size'][1])) != (int(h), int(w)):
        raise ValueError('%s: the mask is %d x %d, its image %d x %d' % (what, seg['size'][0], seg['size'][1], h, w))
    c = seg['counts']
    if isinstance(c, (str, bytes)):
        cnts = rle_from_string(c)
    else:
        raw = np.asarray(c).reshape(-1)
        if raw.size and (raw.dtype.kind not in 'iu' or raw.min() < 0 or raw.max() > 0xFFFFFFFF):
            raise ValueError('%s: counts are non-negative integers below 2^32' % what)
        cnts = raw.astype(np.uint32)
    if int(cnts.sum(dtype=np.int64)) != int(h) * int(w):
        raise ValueError('%s: the counts sum to %d, the image has %d x %d = %d pixels' % (what, int(cnts.sum(dtype=np.int64)), h, w, int(h) * int(w)))
    if len(cnts) > 1 and not cnts[1:].all():
        raise ValueError('%s: an empty run after the first count (the reference\'s own walk stops early on such a mask)' % what)
    return cnts


def rle_from_polys(polys, hw, names=None):
    """rleFrPoly + rleMerge (maskApi.c:139-179, 49-70; cocoeval.py:92-101) on the device: polys[a] = the flat [x0, y0, x1, y1, ...]
    polygons of annotation a, hw (NA,2) its image's h, w -> one uint32 count array per annotation, the reference's.  The host builds
    the offsets -- the upsampled integer vertices and the boundary points per edge, in the same float64 arithmetic as the kernel,
    because they size the walk -- and reads the crossing counts back once (sn_rle_poly_cross, sn_rle_from_polys)."""
    import torch
    from . import hip
    NA = len(polys)
    names = names or ['rle_from_polys: annotation %d' % a for a in range(NA)]
    hw = np.asarray(hw, np.int64).reshape(NA, 2)
    parts, per_ann = [], []
    for a, ann in enumerate(polys):
        if not isinstance(ann, (list, tuple)) or len(ann) == 0:
            raise ValueError('%s: a polygon annotation is a non-empty list of flat coordinate lists' % names[a])
        for q in ann:
            q = np.asarray(q, np.float64).reshape(-1)
            if len(q) < 2 or len(q) % 2 or not np.isfinite(q).all() or np.abs(q).max() >= 2.0 ** 28:
                raise ValueError('%s: a polygon is x0, y0, x1, y1, ... with at least one vertex, finite and below 2^28 in size' % names[a])
            parts.append(q.reshape(-1, 2))
        per_ann.append(len(ann))
    if hw.min() < 1 or (hw[:, 0] * hw[:, 1]).max() >= 2 ** 31:
        raise ValueError('rle_from_polys: every image needs h >= 1, w >= 1 and h * w < 2^31')
    dev = hip.require_gpu()                   # (after the checks: a malformed annotation is reported without a device)
    NP = len(parts)
    ann_off = np.concatenate([[0], np.cumsum(per_ann)])
    poly_off = np.concatenate([[0], np.cumsum([len(q) for q in parts])])
    xy = np.concatenate(parts)
    TV = len(xy)
    xi = np.trunc(5.0 * xy + 0.5).astype(np.int64)            # the C cast (int): truncation toward zero
    nxt = np.arange(1, TV + 1)
    nxt[poly_off[1:] - 1] = poly_off[:-1]                     # the last vertex of a polygon is joined to its first
    d = np.abs(xi[nxt] - xi)
    edge_pt_off = np.concatenate([[0], np.cumsum(np.maximum(d[:, 0], d[:, 1]) + 1)])
    if edge_pt_off[-1] >= 2 ** 31 or TV >= 2 ** 30:
        raise ValueError('rle_from_polys: %d boundary points and %d vertices in one call, 32-bit indexing takes fewer' % (edge_pt_off[-1], TV))
    poly_hw = np.repeat(hw, per_ann, axis=0).astype(np.int32)
    max_hw = int((hw[:, 0] * hw[:, 1]).max())
    i32 = lambda n: torch.empty([max(int(n), 1)], dtype=torch.int32, device=dev)
    d_xy, d_poly_off, d_edge, d_hw = hip.dev(xy), hip.dev(poly_off.astype(np.int32)), hip.dev(edge_pt_off.astype(np.int32)), hip.dev(poly_hw)
    count = i32(NP)
    hip.call('sn_rle_poly_cross', d_xy, d_poly_off, d_edge, d_hw, None, NP, TV, int(edge_pt_off[-1]), max_hw, count, None, hip.stream())
    cross_off = np.concatenate([[0], np.cumsum(count[:NP].cpu().numpy().astype(np.int64))])
    total = int(cross_off[-1])
    if total + NP >= 2 ** 30:
        raise ValueError('rle_from_polys: %d crossings in one call, 32-bit indexing takes fewer' % total)
    d_cross_off, cross = hip.dev(cross_off.astype(np.int32)), i32(total)
    hip.call('sn_rle_poly_cross', d_xy, d_poly_off, d_edge, d_hw, d_cross_off, NP, TV, int(edge_pt_off[-1]), max_hw, None, cross, hip.stream())
    ws = torch.empty(int(hip.query('sn_rle_from_polys_workspace_bytes', total)), dtype=torch.uint8, device=dev)
    part_runs, runs, part_m, ann_m = i32(total + NP), i32(total + NP), i32(NP), i32(NA)
    hip.call('sn_rle_from_polys', cross, d_cross_off, d_hw, hip.dev(ann_off.astype(np.int32)), NP, NA, total, ws, ws.numel(), part_runs,
             part_m, runs, ann_m, hip.stream())
    h_runs, h_m = runs.cpu().numpy().view(np.uint32), ann_m[:NA].cpu().numpy()
    start = cross_off[ann_off[:-1]] + ann_off[:-1]
    return [h_runs[start[a]:start[a] + h_m[a]].copy() for a in range(NA)]


def paste_boxes(rows, h, w, what='paste_boxes'):
    """The box of mask_voc2coco for every detection row (x1, y1, x2, y2, ...): clip_boxes (lib/bbox/bbox_transform.py:35-50) in float64,
    then np.round(...).astype(int) -> (n,4) int.  A box with x2 < x1 or y2 < y1 after that is refused with a ValueError that names
    the detection (the reference's cv2.resize fails on it too)."""
    b = np.array(np.asarray(rows)[:, :4], np.float64).reshape(-1, 4)
    b[:, 0::2] = np.maximum(np.minimum(b[:, 0::2], w - 1), 0)
    b[:, 1::2] = np.maximum(np.minimum(b[:, 1::2], h - 1), 0)
    b = np.round(b).astype(int)
    bad = np.flatnonzero((b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1]))
    if len(bad):
        raise ValueError('%s: detection %d has the box %s after clipping and rounding: x2 < x1 or y2 < y1' % (what, bad[0], b[bad[0]].tolist()))
    return b


def rle_paste(masks, boxes, hw, binary_thresh=0.4):
    """mask_voc2coco (lib/mask/mask_voc2coco.py:39-49) on the device: masks (n, M, M) probabilities, boxes (n,4) int from paste_boxes,
    hw (n,2) each detection's image size -> one uint32 count array per detection: the mask resized to its box (float32 bilinear, the
    resize this project specifies -- include/sniper_hip.h -- NOT pinned to OpenCV), >= float32(binary_thresh), zeros outside the box,
    the whole image run-length encoded column-major.  One read-back: the value changes per detection (sn_rle_paste_count, sn_rle_paste)."""
    import torch
    from . import hip
    dev = hip.require_gpu()
    masks = np.ascontiguousarray(masks, np.float32)
    n, M = masks.shape[0], masks.shape[1]
    assert masks.shape == (n, M, M) and n >= 1, 'masks are (n, M, M)'
    boxes = np.ascontiguousarray(boxes, np.int32).reshape(n, 4)
    hw = np.ascontiguousarray(hw, np.int32).reshape(n, 2)
    ok = (0 <= boxes[:, 0]) & (boxes[:, 0] <= boxes[:, 2]) & (boxes[:, 2] < hw[:, 1]) & (0 <= boxes[:, 1]) & (boxes[:, 1] <= boxes[:, 3]) & (boxes[:, 3] < hw[:, 0])
    if not ok.all():
        raise ValueError('rle_paste: detection %d has the box %s outside its %d x %d image or empty' % (
            np.flatnonzero(~ok)[0], boxes[np.flatnonzero(~ok)[0]].tolist(), hw[np.flatnonzero(~ok)[0], 0], hw[np.flatnonzero(~ok)[0], 1]))
    col_off = np.concatenate([[0], np.cumsum(boxes[:, 2].astype(np.int64) - boxes[:, 0] + 1)])
    max_hw = int((hw[:, 0].astype(np.int64) * hw[:, 1]).max())
    thr = float(np.float32(binary_thresh))
    i32 = lambda k: torch.empty([max(int(k), 1)], dtype=torch.int32, device=dev)
    d_m, d_b, d_hw, d_col = hip.dev(masks), hip.dev(boxes), hip.dev(hw), hip.dev(col_off.astype(np.int32))
    col_pre, det_t = i32(col_off[-1]), i32(n)
    hip.call('sn_rle_paste_count', d_m, d_b, d_hw, d_col, n, M, thr, int(col_off[-1]), max_hw, col_pre, det_t, hip.stream())
    rle_off = np.concatenate([[0], np.cumsum(det_t[:n].cpu().numpy().astype(np.int64) + 1)])
    total = int(rle_off[-1])
    tpos, cnts = i32(total), i32(total)
    hip.call('sn_rle_paste', d_m, d_b, d_hw, d_col, col_pre, hip.dev(rle_off.astype(np.int32)), n, M, thr, int(col_off[-1]), total, max_hw,
             tpos, cnts, hip.stream())
    h_c = cnts[:total].cpu().numpy().view(np.uint32)
    return [h_c[rle_off[i]:rle_off[i + 1]].copy() for i in range(n)]


class COCOSegmResult(COCOBoxResult):
    """COCOBoxResult of a mask evaluation: the same arrays, statistics and summary lines (the reference's summary does not name the
    IoU type); timing names the stages"""
    iou_type = 'segm'


def _pool(rles):
    off = np.zeros(len(rles) + 1, np.int64)
    if len(rles):
        np.cumsum(np.fromiter(map(len, rles), np.int64, len(rles)), out=off[1:])
    cnts = np.concatenate(rles).astype(np.uint32, copy=False) if off[-1] else np.zeros(0, np.uint32)
    return cnts, off


class COCOSegmEvaluator(object):
    """gt: dict over the NG annotations in annotation order -- image (index into image_ids), category (index into cat_ids), area (the
    annotation's own, as in the reference), iscrowd, ignore (optional, 0) and segmentation: per annotation a dict with `size` and
    `counts` as a list (uncompressed RLE) or as a string (compressed: decoded on the host by rle_from_string), or a polygon list.  image_sizes: (I,2)
    h, w.  params: a Params (default: the reference's); useSegm is implied.  chunk_elements bounds the device memory of a chunk: the
    runs of its masks plus the entries of its IoU matrices.

    A segmentation may also be a list of flat polygon coordinate lists: those annotations are converted together on the device
    (rle_from_polys: rleFrPoly and the union of the parts)."""

    def __init__(self, gt, image_ids, cat_ids, image_sizes, params=None, chunk_elements=1 << 23):
        self.params = params or Params()
        if not getattr(self.params, 'useCats', 1):
            raise NotImplementedError('COCOSegmEvaluator: useCats = 0 (category-agnostic evaluation) is not implemented')
        self.image_ids, self.cat_ids = list(image_ids), list(cat_ids)
        I, K = len(self.image_ids), len(self.cat_ids)
        self.image_sizes = np.asarray(image_sizes, np.int64).reshape(I, 2)
        if I and (self.image_sizes.min() < 1 or (self.image_sizes[:, 0] * self.image_sizes[:, 1]).max() >= 2 ** 31):
            raise ValueError('COCOSegmEvaluator: every image needs h >= 1, w >= 1 and h * w < 2^31')
        self.chunk_elements = int(chunk_elements)
        n = len(gt['image'])
        self.gt = {
            'image': np.asarray(gt['image'], np.int64).reshape(n), 'category': np.asarray(gt['category'], np.int64).reshape(n),
            'area': np.asarray(gt['area'], np.float64).reshape(n), 'iscrowd': np.asarray(gt['iscrowd']).reshape(n).astype(np.int64) != 0,
            'ignore': (np.asarray(gt['ignore']).reshape(n).astype(np.int64) != 0) if 'ignore' in gt else np.zeros(n, bool),
        }
        assert n == 0 or (0 <= self.gt['image'].min() and self.gt['image'].max() < I), 'gt image index out of range'
        assert n == 0 or (0 <= self.gt['category'].min() and self.gt['category'].max() < K), 'gt category index out of range'
        assert len(gt['segmentation']) == n, '%d segmentations for %d annotations' % (len(gt['segmentation']), n)
        self.gt_rle = []
        for a, seg in enumerate(gt['segmentation']):
            h, w = self.image_sizes[self.gt['image'][a]]
            if isinstance(seg, (list, tuple)):
                self.gt_rle.append(None)              # polygons: converted together on the device, below
            else:
                self.gt_rle.append(rle_counts(seg, h, w, 'COCOSegmEvaluator: annotation %d' % a))
        poly = [a for a, r in enumerate(self.gt_rle) if r is None]
        if poly:
            rles = rle_from_polys([gt['segmentation'][a] for a in poly], self.image_sizes[self.gt['image'][poly]],
                                  ['COCOSegmEvaluator: annotation %d' % a for a in poly])
            for a, r in zip(poly, rles):
                self.gt_rle[a] = r

    @classmethod
    def from_roidb(cls, roidb, num_classes, params=None, **kw):
        """Ground truth = the roidb rows with gt_classes > 0: the mask of row j is roidb[i]['gt_masks'][j] (the polygon lists of
        the training roidb, or an RLE dict), the image size roidb[i]['height'] / ['width'], area =
        roidb[i]['gt_areas'] where present, else the mask's rleArea from the device (sn_rle_stats), iscrowd = roidb[i]['gt_iscrowd']
        where present, else 0.  Image ids are 1.., category ids 1..num_classes-1, annotation ids follow the roidb order."""
        img, cat, area, crowd, seg = [], [], [], [], []
        for i, r in enumerate(roidb):
            classes = np.asarray(r['gt_classes'])
            keep = np.flatnonzero(classes > 0)
            img.append(np.full(len(keep), i, np.int64))
            cat.append(classes[keep].astype(np.int64) - 1)
            area.append(np.asarray(r['gt_areas'], np.float64)[keep] if 'gt_areas' in r else np.full(len(keep), np.nan))
            crowd.append(np.asarray(r['gt_iscrowd'])[keep].astype(np.int64) if 'gt_iscrowd' in r else np.zeros(len(keep), np.int64))
            seg.extend(r['gt_masks'][j] for j in keep)
        cat0 = lambda parts, dt: np.concatenate(parts) if parts else np.zeros((0,), dt)
        gt = {'image': cat0(img, np.int64), 'category': cat0(cat, np.int64), 'area': cat0(area, np.float64), 'iscrowd': cat0(crowd, np.int64),
              'segmentation': seg}
        ev = cls(gt, range(1, len(roidb) + 1), range(1, num_classes), [(r['height'], r['width']) for r in roidb], params, **kw)
        missing = np.flatnonzero(np.isnan(ev.gt['area']))
        if len(missing):
            ev.gt['area'][missing] = ev.mask_areas([ev.gt_rle[n] for n in missing], ev.image_sizes[ev.gt['image'][missing]])
        return ev

    @staticmethod
    def mask_areas(rles, hw):
        """rleArea of every mask, on the device (sn_rle_stats) -> (N) float64"""
        import torch
        from . import hip
        dev = hip.require_gpu()
        cnts, off = _pool(rles)
        hw = np.asarray(hw, np.int64).reshape(len(rles), 2)
        rows = torch.empty((len(rles), 6), dtype=torch.float64, device=dev)
        cum = torch.empty((max(int(off[-1]), 1), 2), dtype=torch.int32, device=dev)
        d_c = hip.dev(cnts.view(np.int32)) if len(cnts) else torch.zeros(1, dtype=torch.int32, device=dev)
        hip.call('sn_rle_stats', d_c, hip.dev(off.astype(np.int32)), hip.dev(hw.astype(np.int32)), None, len(rles), int(off[-1]),
                 int((hw[:, 0] * hw[:, 1]).max()), rows, cum, hip.stream())
        return rows[:, 5].cpu().numpy()

    # ---- detections -----------------------------------------------------------------------------
    def convert_detections(self, all_boxes, all_masks, binary_thresh=0.4):
        """-> (scores (ND) float64, UNROUNDED as coco.py:57 leaves them for segm; the masks' counts, one uint32 array per detection; the
        (K, I) row counts), all in class-major, image, row order -- the order of the reference's result list.  A cell of all_masks is
        the (n, M, M) probabilities of the cell's boxes -- pasted on the device, all cells of one M in one rle_paste call -- or a list
        of n RLE dicts, taken as they are."""
        K, I = len(self.cat_ids), len(self.image_ids)
        counts = _cell_counts(all_boxes, K, I)
        assert len(all_masks) == K + 1, 'all_masks[class][image]: %d classes (with the background) for %d categories' % (len(all_masks), K)
        scores, rles, pending = [], [], {}
        for k in range(K):
            assert len(all_masks[k + 1]) == I, 'all_masks[%d] has %d images, the ground truth %d' % (k + 1, len(all_masks[k + 1]), I)
            for i in np.flatnonzero(counts[k]):
                rows, cell = all_boxes[k + 1][i], all_masks[k + 1][i]
                rows = np.asarray(rows.cpu() if hasattr(rows, 'cpu') else rows).reshape(-1, 5)
                if len(cell) != len(rows):
                    raise ValueError('COCOSegmEvaluator: all_masks[%d][%d] has %d masks, all_boxes[%d][%d] %d rows' % (k + 1, i, len(cell), k + 1, i, len(rows)))
                h, w = self.image_sizes[i]
                scores.append(rows[:, 4].astype(np.float64))
                if isinstance(cell, (list, tuple)):
                    rles.extend(rle_counts(seg, h, w, 'COCOSegmEvaluator: detection %d of all_masks[%d][%d]' % (n, k + 1, i)) for n, seg in enumerate(cell))
                    continue
                prob = np.asarray(cell.cpu() if hasattr(cell, 'cpu') else cell)
                if prob.ndim != 3 or prob.shape[1] != prob.shape[2]:
                    raise ValueError('COCOSegmEvaluator: all_masks[%d][%d] is neither a list of RLE dicts nor (n, M, M) probabilities' % (k + 1, i))
                box = paste_boxes(rows, h, w, 'COCOSegmEvaluator: all_boxes[%d][%d]' % (k + 1, i))
                slot = pending.setdefault(prob.shape[1], ([], [], [], []))
                slot[0].append(prob.astype(np.float32, copy=False)), slot[1].append(box), slot[2].append(np.tile([[h, w]], (len(rows), 1)))
                slot[3].extend(range(len(rles), len(rles) + len(rows)))
                rles.extend([None] * len(rows))
        for prob, box, hw, where in pending.values():
            for n, r in zip(where, rle_paste(np.concatenate(prob), np.concatenate(box), np.concatenate(hw), binary_thresh)):
                rles[n] = r
        return (np.concatenate(scores) if scores else np.zeros(0)), rles, counts

    def _chunks(self, cost):
        """problem ranges [p0, p1) whose summed cost stays within chunk_elements (a single problem over it is a chunk of its own)"""
        cum = np.concatenate([[0], np.cumsum(cost)])
        out, p0, P = [], 0, len(cost)
        while p0 < P:
            p1 = int(np.searchsorted(cum, cum[p0] + self.chunk_elements, side='right')) - 1
            p1 = min(max(p1, p0 + 1), P)
            out.append((p0, p1))
            p0 = p1
        return out

    def evaluate(self, all_boxes, all_masks, binary_thresh=0.4, return_matches=False, return_rles=False):
        """all_boxes[class][image] = (n,5) rows x1, y1, x2, y2, score; all_masks[class][image] = a list of n RLE dicts (class 0 =
        background) or the (n, M, M) mask probabilities of those rows, pasted into the image at binary_thresh (rle_paste)
        -> COCOSegmResult.
        return_matches adds result.matches (sn_coco_match_iou's outputs, the offsets, the IoU matrices as iou / iou_off and the
        rows of sn_rle_stats), return_rles adds result.rles (the counts of every detection and annotation in problem order)."""
        import torch
        from . import hip
        p = self.params
        dev = hip.require_gpu()
        iou_thrs, rec_thrs = np.asarray(p.iouThrs, np.float64), np.asarray(p.recThrs, np.float64)
        area_rng = np.asarray(p.areaRng, np.float64).reshape(-1, 2)
        max_dets = np.asarray(sorted(p.maxDets), np.int32)
        T, R, A, M, K = len(iou_thrs), len(rec_thrs), len(area_rng), len(max_dets), len(self.cat_ids)
        max_det = int(max_dets[-1])
        t0 = _now(torch)
        scores, dt_rle, counts = self.convert_detections(all_boxes, all_masks, binary_thresh)
        ND, NG = len(dt_rle), len(self.gt_rle)
        pr = _problem_offsets(counts, self.gt['category'], self.gt['image'])
        pr['kp_off'] = _offsets(np.minimum(pr.pop('dt_counts'), max_det))
        P = pr['P']
        if P == 0:                                    # nothing to evaluate: every category is absent
            return COCOSegmResult(-np.ones((T, R, K, A, M)), -np.ones((T, K, A, M)), p, self.cat_ids)
        lim = np.zeros(5, np.int32)
        hip.call('sn_rle_limits', lim)
        if pr['max_dt'] > lim[0] or pr['max_gt'] > lim[1]:          # sn_coco_match_iou would refuse the chunk: say so before any launch
            raise ValueError('COCOSegmEvaluator: a problem has %d detections and a problem has %d masks of ground truth; '
                             'sn_coco_match_iou takes at most %d and %d' % (pr['max_dt'], pr['max_gt'], lim[0], lim[1]))
        NK = int(pr['kp_off'][-1])
        o = pr['gt_order']
        gt_rle = [self.gt_rle[n] for n in o]
        flags = (self.gt['iscrowd'][o].astype(np.uint8) | (self.gt['ignore'][o].astype(np.uint8) << 1)) if NG else np.zeros(1, np.uint8)
        gt_area = self.gt['area'][o] if NG else np.zeros(1)
        kk, ii = np.nonzero(counts)
        dt_hw = np.repeat(self.image_sizes[ii], counts[kk, ii], axis=0).astype(np.int32).reshape(-1, 2)
        gt_hw = self.image_sizes[self.gt['image'][o]].astype(np.int32).reshape(-1, 2)
        d_cnts, d_roff = _pool(dt_rle)
        g_cnts, g_roff = _pool(gt_rle)
        dt_off, gt_off = pr['dt_off'].astype(np.int64), pr['gt_off'].astype(np.int64)
        pairs = np.diff(dt_off) * np.diff(gt_off)
        chunks = self._chunks(np.diff(d_roff[dt_off]) + np.diff(g_roff[gt_off]) + pairs)
        kept_per_cat = np.diff(pr['kp_off'][pr['cat_off']].astype(np.int64))
        t1 = _now(torch)
        empty = lambda dtype, *shape: torch.empty([max(int(np.prod(shape)), 1)], dtype=dtype, device=dev)
        d_dt, d_gt = torch.zeros((max(ND, 1), 6), dtype=torch.float64, device=dev), torch.zeros((max(NG, 1), 6), dtype=torch.float64, device=dev)
        d_area, d_flags = hip.dev(gt_area), hip.dev(flags)
        d_dt_off, d_gt_off, d_kp_off, d_cat_off = (hip.dev(pr[k]) for k in ('dt_off', 'gt_off', 'kp_off', 'cat_off'))
        d_iou_thr, d_rec, d_rng = hip.dev(iou_thrs), hip.dev(rec_thrs), hip.dev(area_rng)
        dt_rank, dt_match, dt_ignore = empty(torch.int32, NK), empty(torch.int32, A, T, NK), empty(torch.uint8, A, T, NK)
        gt_match, gt_ignore = empty(torch.int32, A, T, NG), empty(torch.uint8, A, NG)
        precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
        recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
        ws = torch.empty(int(hip.query('sn_coco_accumulate_workspace_bytes', NK, T, A)), dtype=torch.uint8, device=dev)
        tm = {'host_s': t1 - t0, 'upload_s': _now(torch) - t1, 'stats_s': 0., 'iou_s': 0., 'match_s': 0.}
        ious, iou_offs = [], [np.zeros(1, np.int64)]

        def upload(cnts, roff, hw, lo, hi, score):
            """masks [lo, hi) of a pool -> the device operands of sn_rle_stats (counts, relative run offsets, sizes, scores, cum2)"""
            if hi == lo:
                return None
            rel = (roff[lo:hi + 1] - roff[lo]).astype(np.int32)
            total = int(rel[-1])
            d_c = hip.dev(cnts[roff[lo]:roff[hi]].view(np.int32)) if total else empty(torch.int32, 1)
            return (d_c, hip.dev(rel), hip.dev(hw[lo:hi]), hip.dev(score[lo:hi]) if score is not None else None, hi - lo, total,
                    int((hw[lo:hi, 0].astype(np.int64) * hw[lo:hi, 1]).max()), empty(torch.int32, total, 2))

        for p0, p1 in chunks:
            tc = _now(torch)
            dl, dh, gl, gh = int(dt_off[p0]), int(dt_off[p1]), int(gt_off[p0]), int(gt_off[p1])
            up_d, up_g = upload(d_cnts, d_roff, dt_hw, dl, dh, scores), upload(g_cnts, g_roff, gt_hw, gl, gh, None)
            io = np.concatenate([[0], np.cumsum(pairs[p0:p1])])
            n_pairs = int(io[-1])
            assert n_pairs < 2 ** 31, 'a chunk has %d (detection, annotation) pairs: lower chunk_elements' % n_pairs
            d_io, iou = hip.dev(io.astype(np.int32)), empty(torch.float64, n_pairs)
            tu = _now(torch)
            for up, rows, lo in ((up_d, d_dt, dl), (up_g, d_gt, gl)):
                if up is not None:
                    hip.call('sn_rle_stats', up[0], up[1], up[2], up[3], up[4], up[5], up[6], rows[lo:], up[7], hip.stream())
            ts = _now(torch)
            if n_pairs:
                hip.call('sn_rle_iou', up_d[7], up_d[1], d_dt[dl:], up_g[7], up_g[1], d_gt[gl:], d_flags[gl:], d_dt_off[p0:], d_gt_off[p0:],
                         d_io, p1 - p0, n_pairs, iou, hip.stream())
            ti = _now(torch)
            hip.call('sn_coco_match_iou', d_dt, d_dt_off[p0:], d_kp_off[p0:], d_area, d_flags, d_gt_off[p0:], iou, d_io, d_iou_thr, d_rng,
                     p1 - p0, T, A, max_det, int(np.diff(dt_off[p0:p1 + 1]).max()), int(np.diff(gt_off[p0:p1 + 1]).max()), NK, NG,
                     dt_rank, dt_match, dt_ignore, gt_match, gt_ignore, hip.stream())
            te = _now(torch)
            tm['upload_s'] += tu - tc
            tm['stats_s'] += ts - tu
            tm['iou_s'] += ti - ts
            tm['match_s'] += te - ti
            if return_matches:
                ious.append(iou[:n_pairs].cpu().numpy())
                iou_offs.append(io[1:] + iou_offs[-1][-1])
        t2 = _now(torch)
        hip.call('sn_coco_accumulate', d_dt, d_dt_off, d_kp_off, d_gt_off, d_cat_off, dt_rank, dt_match, dt_ignore, gt_ignore, d_rec,
                 max_dets, P, K, T, A, M, R, max_det, int(kept_per_cat.max()), NK, NG, ws, ws.numel(), precision, recall, hip.stream())
        t3 = _now(torch)
        h_precision, h_recall = precision.cpu().numpy(), recall.cpu().numpy()
        t4 = _now(torch)
        # seconds: host = counts of the masks, pools, CSR offsets; upload = allocations + copies to the device (all chunks); stats =
        # sn_rle_stats, iou = sn_rle_iou, match = sn_coco_match_iou (all chunks); accumulate = sn_coco_accumulate; download = precision
        # + recall to the host
        tm.update({'accumulate_s': t3 - t2, 'download_s': t4 - t3, 'kernels_s': tm['stats_s'] + tm['iou_s'] + tm['match_s'] + t3 - t2,
                   'problems': P, 'detections': ND, 'kept': NK, 'boxes': NG, 'chunks': len(chunks), 'pairs': int(pairs.sum()),
                   'runs': int(d_roff[-1] + g_roff[-1])})
        res = COCOSegmResult(h_precision, h_recall, p, self.cat_ids, tm)
        if return_matches:
            res.matches = dict(pr, NK=NK, dt_rank=dt_rank[:NK].cpu().numpy(), dt_match=dt_match[:A * T * NK].reshape(A, T, NK).cpu().numpy(),
                               dt_ignore=dt_ignore[:A * T * NK].reshape(A, T, NK).cpu().numpy(),
                               gt_match=gt_match[:A * T * NG].reshape(A, T, NG).cpu().numpy(),
                               gt_ignore=gt_ignore[:A * NG].reshape(A, NG).cpu().numpy(), dt=d_dt[:ND].cpu().numpy(), gt=d_gt[:NG].cpu().numpy(),
                               iou=np.concatenate(ious) if ious else np.zeros(0), iou_off=np.concatenate(iou_offs))
        if return_rles:
            res.rles = {'dt': dt_rle, 'gt': gt_rle}
        return res


def evaluate_sds(all_boxes, all_masks, roidb, num_classes, binary_thresh=0.4, params=None):
    """`imdb.evaluate_sds(all_boxes, all_masks)` of the reference's mask test run in one call, for run-length encoded masks on both
    sides: ground truth from the roidb (COCOSegmEvaluator.from_roidb), detections as lists of RLE dicts beside all_boxes ->
    COCOSegmResult; print(result.summary()) gives the reference's twelve lines"""
    return COCOSegmEvaluator.from_roidb(roidb, num_classes, params).evaluate(all_boxes, all_masks, binary_thresh=binary_thresh)


# ---- PASCAL VOC masks ------------------------------------------------------------------------------------
# The fourth cell of the grid (two data sets, two annotation types): the mask AP of PASCAL VOC / SBD, voc_eval_sds
# (lib/dataset/pascal_voc_eval.py:184-272) with mask_overlap (lib/mask/mask_transform.py:40-70).  It is NOT COCOeval with other
# parameters: the overlap is taken between the thresholded (M, M) map resized to its rounded box and the cropped instance mask in its
# bound (no image size, no RLE, no bounding-box gate), a match needs ov >= t, only the first instance of maximal overlap is looked
# at, an instance already detected makes the detection a false positive, there is no difficult flag, and the AP is always the
# 11-point one.  sn_vocsds_mask_iou and sn_vocsds_match_iou (sniper_amd/csrc/voc_segm.hip) do the overlaps and
# the matching, sn_voc_accumulate the curves, unchanged.  The host rounds the boxes and builds the pools and offsets (numpy).
__all__ += ['VOCSegmEvaluator', 'VOCSegmResult', 'evaluate_sds_voc', 'round_mask_boxes']


def round_mask_boxes(rows, what='round_mask_boxes'):
    """np.round(box).astype(int) of voc_eval_sds (pascal_voc_eval.py:233) for every detection row (x1, y1, x2, y2, ...), taken in
    float64 as the reference's new_boxes holds them -> (n,4) int32.  Nothing is clipped: the reference knows no image size here.  A box
    with x2 < x1 or y2 < y1 after the rounding is refused with a ValueError that names the detection (the reference's cv2.resize fails
    on it too)."""
    b = np.round(np.array(np.asarray(rows)[:, :4], np.float64).reshape(-1, 4))
    if len(b) and np.abs(b).max() >= 2 ** 30:
        raise ValueError('%s: detection %d has a coordinate of magnitude 2^30 or more' % (what, int(np.argmax(np.abs(b).max(axis=1)))))
    b = b.astype(np.int32)
    bad = np.flatnonzero((b[:, 2] < b[:, 0]) | (b[:, 3] < b[:, 1]))
    if len(bad):
        raise ValueError('%s: detection %d has the box %s after rounding: x2 < x1 or y2 < y1' % (what, bad[0], b[bad[0]].tolist()))
    return b


class VOCSegmResult(VOCBoxResult):
    """VOCBoxResult of a mask evaluation: ap07 (what voc_eval_sds returns), ap_area (T,K), ap = ap07, mean_ap (T,), npos (K,),
    summary() (the box evaluation's lines; voc_eval_sds always takes the 11-point metric), timing per stage"""

    def __init__(self, ap07, ap_area, npos, class_names, thresholds, timing=None):
        VOCBoxResult.__init__(self, ap07, ap_area, npos, class_names, True, thresholds, timing)


class VOCSegmEvaluator(object):
    """records[i]: the list parse_inst (pascal_voc_eval.py:275-318) returns for image i -- dicts with `mask` (bool (h, w), the
    instance cropped to its bound), `mask_bound` (x1, y1, x2, y2; rounded here as the reference rounds it, np.round(...).astype(int))
    and `mask_cls` (1 .. K, the index into the class list with the background at 0).  class_names: the K foreground classes (a
    leading '__background__' is dropped).  A mask whose shape is not its bound's is refused with a ValueError."""

    def __init__(self, records, num_images, class_names, thresholds=(0.5, 0.7)):
        names = list(class_names)
        self.class_names = names[1:] if names and names[0] == '__background__' else names
        self.num_images = int(num_images)
        self.thresholds = tuple(float(t) for t in thresholds)
        assert len(records) == self.num_images, '%d records for %d images' % (len(records), self.num_images)
        K = len(self.class_names)
        img, cat, bound, bits, area = [], [], [], [], []
        for i, rec in enumerate(records):
            for j, inst in enumerate(rec):
                b = np.round(np.asarray(inst['mask_bound'], np.float64).reshape(4)).astype(np.int64)
                m = np.asarray(inst['mask'])
                c = int(inst['mask_cls'])
                if m.ndim != 2 or m.shape != (b[3] - b[1] + 1, b[2] - b[0] + 1):
                    raise ValueError('VOCSegmEvaluator: instance %d of image %d has a mask of shape %s in the bound %s' % (j, i, m.shape, b.tolist()))
                if not 1 <= c <= K:
                    raise ValueError('VOCSegmEvaluator: instance %d of image %d has mask_cls %d, outside 1 .. %d' % (j, i, c, K))
                if np.abs(b).max() >= 2 ** 30:
                    raise ValueError('VOCSegmEvaluator: instance %d of image %d has a coordinate of magnitude 2^30 or more' % (j, i))
                m = (m != 0).astype(np.uint8).reshape(-1)
                img.append(i); cat.append(c - 1); bound.append(b); bits.append(m); area.append(int(m.sum()))
        n = len(img)
        self.gt = {'image': np.array(img, np.int64).reshape(n), 'category': np.array(cat, np.int64).reshape(n),
                   'bound': np.array(bound, np.int32).reshape(n, 4), 'area': np.array(area, np.int32).reshape(n), 'bits': bits}

    def _pool(self, order):
        """the instances' bitmaps in CSR order -> (bits (pool,) uint8, pix_off (NG+1) int64)"""
        parts = [self.gt['bits'][g] for g in order]
        off = np.zeros(len(parts) + 1, np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off

    def convert_detections(self, all_boxes, all_masks):
        """-> (boxes (ND,4) int32 rounded, scores (ND,) float64, masks (ND,M,M) float32, (K, I) row counts), class-major, image, row.
        A box that rounds to x2 < x1 or y2 < y1 is a ValueError naming its class, image and row."""
        K, I = len(self.class_names), self.num_images
        counts = _cell_counts(all_boxes, K, I)
        assert len(all_masks) == K + 1, 'all_masks[class][image]: %d classes (with the background) for %d categories' % (len(all_masks), K)
        host = lambda d: np.asarray(d.cpu() if hasattr(d, 'cpu') else d)
        cells, rows, maps, M = [], [], [], None
        for k in range(K):
            assert len(all_masks[k + 1]) == I, 'all_masks[%d] has %d images, the ground truth %d' % (k + 1, len(all_masks[k + 1]), I)
            for i in np.flatnonzero(counts[k]):
                r, m = host(all_boxes[k + 1][i]).reshape(-1, 5), host(all_masks[k + 1][i])
                if m.ndim != 3 or m.shape[0] != len(r) or m.shape[1] != m.shape[2] or (M is not None and m.shape[1] != M):
                    raise ValueError('VOCSegmEvaluator: all_masks[%d][%d] has the shape %s for %d boxes%s' % (
                        k + 1, i, m.shape, len(r), '' if M is None else ' and M = %d' % M))
                M = m.shape[1]
                cells.append((k + 1, i))
                rows.append(r.astype(np.float64))          # exact: the reference's new_boxes is a float64 array too
                maps.append(m)
        if not rows:
            return np.zeros((0, 4), np.int32), np.zeros(0, np.float64), np.zeros((0, 1, 1), np.float32), counts
        raw = np.concatenate(rows, axis=0)
        try:
            boxes = round_mask_boxes(raw)
        except ValueError:                                 # name the cell and the row within it
            for (c, i), r in zip(cells, rows):
                try:
                    round_mask_boxes(r)
                except ValueError as e:
                    raise ValueError('VOCSegmEvaluator: class %d, image %d: %s' % (c, i, e))
            raise
        masks = np.ascontiguousarray(np.concatenate(maps, axis=0), np.float32)
        return boxes, np.ascontiguousarray(raw[:, 4]), masks, counts

    def evaluate(self, all_boxes, all_masks, binary_thresh=0.4, return_matches=False):
        """all_boxes[class][image] = (n,5) rows x1, y1, x2, y2, score and all_masks[class][image] = (n,M,M) probabilities as
        mask_inference.predict_masks returns them (class 0 = background) -> VOCSegmResult.  return_matches adds result.matches: the
        offsets, the rounded boxes, dt_area, iou / iou_off, the outputs of sn_vocsds_match_iou, order, rec, prec and cls_off."""
        import torch
        from . import hip
        dev = hip.require_gpu()
        thrs = np.asarray(self.thresholds, np.float64)
        T, K = len(thrs), len(self.class_names)
        t0 = _now(torch)
        boxes, scores, masks, counts = self.convert_detections(all_boxes, all_masks)
        ND, NG, M = len(boxes), len(self.gt['image']), masks.shape[1]
        pr = _problem_offsets(counts, self.gt['category'], self.gt['image'])
        P = pr['P']
        if P == 0:                                    # neither detections nor instances: every AP is 0, as the reference's
            return VOCSegmResult(np.zeros((T, K)), np.zeros((T, K)), np.zeros(K, np.int32), self.class_names, self.thresholds)
        o = pr['gt_order']
        bits, pix_off = self._pool(o)
        gcount = np.diff(pr['gt_off'].astype(np.int64))
        iou_off64 = np.concatenate([[0], np.cumsum(pr['dt_counts'].astype(np.int64) * gcount)])
        if iou_off64[-1] >= 2 ** 31:
            raise ValueError('VOCSegmEvaluator: %d (detection, instance) pairs in one call, 2^31 at the most' % iou_off64[-1])
        n_pairs = int(iou_off64[-1])
        pixels = (boxes[:, 2].astype(np.int64) - boxes[:, 0] + 1) * (boxes[:, 3].astype(np.int64) - boxes[:, 1] + 1)
        if ND and pixels.max() >= 2 ** 31:
            raise ValueError('VOCSegmEvaluator: detection %d has a box of %d pixels, below 2^31 required' % (int(np.argmax(pixels)), pixels.max()))
        cls_off = pr['dt_off'][pr['cat_off']]
        per_class = np.diff(cls_off.astype(np.int64))
        ap07_thrs = np.arange(0., 1.1, 0.1)
        t1 = _now(torch)
        some = lambda a, dtype: hip.dev(a) if len(a) else torch.zeros((4,), dtype=dtype, device=dev)
        d_score = some(scores, torch.float64)
        d_bits, d_pix, d_bound = some(bits, torch.uint8), hip.dev(pix_off), some(self.gt['bound'][o], torch.int32)
        d_area, d_zero = some(self.gt['area'][o], torch.int32), torch.zeros((max(NG, 1),), dtype=torch.uint8, device=dev)
        d_dt_off, d_gt_off, d_cat_off = hip.dev(pr['dt_off']), hip.dev(pr['gt_off']), hip.dev(pr['cat_off'])
        d_iou_off, d_thr = hip.dev(iou_off64.astype(np.int32)), hip.dev(thrs)
        empty = lambda dtype, *shape: torch.empty([max(int(np.prod(shape)), 1)], dtype=dtype, device=dev)
        dt_area, iou = empty(torch.int32, ND), empty(torch.float64, n_pairs)
        dt_best, dt_iou = empty(torch.int32, ND), empty(torch.float64, ND)
        dt_tp, dt_fp, gt_det = empty(torch.uint8, T, ND), empty(torch.uint8, T, ND), empty(torch.int32, T, NG)
        order, rec, prec = empty(torch.int32, ND), empty(torch.float64, T, ND), empty(torch.float64, T, ND)
        npos = torch.empty((K,), dtype=torch.int32, device=dev)
        ap07 = torch.empty((T, K), dtype=torch.float64, device=dev)
        ap_area = torch.empty((T, K), dtype=torch.float64, device=dev)
        ws = torch.empty(int(hip.query('sn_voc_accumulate_workspace_bytes', ND, T)), dtype=torch.uint8, device=dev)
        if ND:
            d_masks, d_box = hip.dev(masks), hip.dev(boxes)
        t2 = _now(torch)
        if ND:                                        # without detections there is no overlap to take
            hip.call('sn_vocsds_mask_iou', d_masks, d_box, d_dt_off, d_bits, d_pix, d_bound, d_area, d_gt_off, d_iou_off, P, M,
                     float(np.float32(binary_thresh)), pr['max_gt'], ND, NG, n_pairs, int(pixels.max()), dt_area, iou, hip.stream())
        ti = _now(torch)
        hip.call('sn_vocsds_match_iou', d_score, d_dt_off, d_gt_off, iou, d_iou_off, d_thr, P, T, pr['max_dt'], pr['max_gt'], ND, NG,
                 dt_best, dt_iou, dt_tp, dt_fp, gt_det, hip.stream())
        tm = _now(torch)
        hip.call('sn_voc_accumulate', d_score, d_dt_off, d_gt_off, d_cat_off, d_zero, dt_tp, dt_fp, ap07_thrs, P, K, T,
                 int(per_class.max()), ND, NG, ws, ws.numel(), order, rec, prec, npos, ap07, ap_area, hip.stream())
        t3 = _now(torch)
        h_ap07, h_area, h_npos = ap07.cpu().numpy(), ap_area.cpu().numpy(), npos.cpu().numpy()
        matches = None
        if return_matches:
            rd = lambda x, *shape: x[:int(np.prod(shape))].reshape(shape).cpu().numpy()
            matches = dict(pr, cls_off=cls_off, dt_box=boxes, dt_score=scores, iou_off=iou_off64.astype(np.int32), dt_area=rd(dt_area, ND),
                           iou=rd(iou, n_pairs), dt_best=rd(dt_best, ND), dt_iou=rd(dt_iou, ND), dt_tp=rd(dt_tp, T, ND),
                           dt_fp=rd(dt_fp, T, ND), gt_det=rd(gt_det, T, NG), order=rd(order, ND), rec=rd(rec, T, ND), prec=rd(prec, T, ND))
        t4 = _now(torch)
        # seconds: host = rounding, pools and CSR offsets; upload = allocations + copies to the device; mask_iou, match, accumulate =
        # the three entry points; download = the APs and npos (and the matches, if asked for)
        res = VOCSegmResult(h_ap07, h_area, h_npos, self.class_names, self.thresholds,
                            {'host_s': t1 - t0, 'upload_s': t2 - t1, 'kernels_s': t3 - t2, 'mask_iou_s': ti - t2, 'match_s': tm - ti,
                             'accumulate_s': t3 - tm, 'download_s': t4 - t3, 'problems': P, 'detections': ND, 'instances': NG,
                             'pairs': n_pairs})
        if matches is not None:
            res.matches = matches
        return res


def evaluate_sds_voc(all_boxes, all_masks, records, num_classes, class_names=None, binary_thresh=0.4):
    """The mask AP of a PASCAL VOC / SBD test run in one call: voc_eval_sds per class at 0.5 and 0.7.  records[i] = parse_inst's list
    for image i, detections and masks as Tester.aggregate and mask_inference.predict_masks return them -> VOCSegmResult;
    print(result.summary()) gives the AP lines"""
    if class_names is None:
        class_names = VOC_CLASSES if num_classes == len(VOC_CLASSES) + 1 else ['class%d' % c for c in range(1, num_classes)]
    names = list(class_names)
    names = names[1:] if names and names[0] == '__background__' else names
    assert len(names) == num_classes - 1, '%d class names for %d classes with the background' % (len(names), num_classes)
    return VOCSegmEvaluator(records, len(records), names).evaluate(all_boxes, all_masks, binary_thresh=binary_thresh)
