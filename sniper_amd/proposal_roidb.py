"""The proposal roidb: what lib/dataset/imdb.py:81-204, 291-419 does between the `<name>_rpn.pkl` that Tester.extract_proposals
writes and the roidb that the negative-chip training run reads (main_train.py:60-64, load_proposal_roidb(proposal='rpn',
append_gt=True)).  The reference's method names and signatures, as plain functions and as `ProposalRoidbMixin`.

The per-image work runs on the device (csrc/prop_roidb.hip), all images of a call in ragged launches:
  load_rpn_data               nmsp at 0.7 over every image             -> sn_prop_nms
  create_roidb_from_box_list  bbox_overlaps + max / argmax per image   -> sn_prop_assign
  evaluate_recall             the greedy one-to-one matching           -> sn_prop_recall
What stays on the host: the pickles, the dense (N, num_classes) `gt_overlaps` rows (one non-zero value per row, built from the
device's (max_ov, max_cls)), the area-range membership (numpy, in the arrays' own dtype as the reference computes it), the recalls,
their mean and the strings.  There is no host fallback: without the library or a device a call fails.

Two things the reference leaves open and this module defines: equal scores in the NMS order rank the LATER row first (the
reference's `argsort()[::-1]` on an unstable sort), and an image with more than `limits()['max_gt']` ground-truth boxes is refused
with a ValueError that names it."""
import os
import pickle
import time

import numpy as np

AREA_NAMES = ['all', '0-25', '25-50', '50-100', '100-200', '200-300', '300-inf']
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 25 ** 2], [25 ** 2, 50 ** 2], [50 ** 2, 100 ** 2],
               [100 ** 2, 200 ** 2], [200 ** 2, 300 ** 2], [300 ** 2, 1e5 ** 2]]
CHUNK_BYTES = 64 << 20          # device bytes of input rows per launch group: a training set needs no single allocation
CHUNK_IMAGES = 32768            # (sn_prop_nms takes at most 65535 images a call)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    assert off[-1] < 2 ** 31 // 5, 'a chunk of %d rows' % off[-1]
    return off.astype(np.int32)


def _stack(arrays, width, dtype):
    if not len(arrays):
        return np.zeros((0, width), dtype)
    return np.ascontiguousarray(np.concatenate([np.asarray(a, dtype).reshape(-1, width) for a in arrays], axis=0))


def _up(arr, dev):
    """host array -> device tensor; an empty array still gets an address (the entry points refuse NULL)"""
    import torch
    if arr.size == 0:
        return torch.zeros(16, dtype=torch.uint8, device=dev)
    return torch.from_numpy(arr).to(dev)


class ProposalRoidbEvaluator(object):
    """The device stages, one method per kernel family; each takes per-image lists, cuts them into chunks of CHUNK_BYTES, and per
    chunk builds the host rows and offsets, uploads, launches and downloads.  `timing` accumulates the seconds of each stage
    (host / upload / kernels / download) when a dict is passed."""

    def __init__(self, chunk_bytes=CHUNK_BYTES):
        import ctypes
        from . import hip
        out = (ctypes.c_int32 * 6)()
        hip.lib().call('sn_prop_limits', out)
        self.max_gt, self.max_t, self.assign_block, self.recall_threads, self.nms_tile, self.sort_tile = [int(v) for v in out]
        self.chunk_bytes = int(chunk_bytes)
        self._ws = None

    def limits(self):
        return {'max_gt': self.max_gt, 'max_t': self.max_t, 'assign_block': self.assign_block, 'recall_threads': self.recall_threads,
                'nms_tile': self.nms_tile, 'sort_tile': self.sort_tile}

    # ---- plumbing ------------------------------------------------------------------------------------------------------------
    def _chunks(self, row_bytes):
        """row_bytes (I): device bytes of every image -> [(i0, i1)], each within the byte budget (a single larger image alone)"""
        out, i0, acc = [], 0, 0
        for i, b in enumerate(row_bytes):
            if i > i0 and (acc + b > self.chunk_bytes or i - i0 >= CHUNK_IMAGES):
                out.append((i0, i))
                i0, acc = i, 0
            acc += int(b)
        if len(row_bytes) > i0:
            out.append((i0, len(row_bytes)))
        return out

    def check_gt(self, gt_counts, names=None):
        """the ValueError of an image over the limit, before anything is launched"""
        for i, g in enumerate(gt_counts):
            if g > self.max_gt:
                raise ValueError('image %d%s has %d ground-truth boxes, the device matches at most %d per image'
                                 % (i, ' (%s)' % (names[i],) if names is not None else '', g, self.max_gt))

    @staticmethod
    def _tick(timing, key, t0, sync=False):
        if timing is None:
            return t0
        if sync:
            import torch
            torch.cuda.synchronize()
        t1 = time.perf_counter()
        timing[key] = timing.get(key, 0.0) + (t1 - t0)
        return t1

    # ---- stages --------------------------------------------------------------------------------------------------------------
    def nms(self, box_list, thresh=0.7, timing=None):
        """[(n,5) float32 rows] -> [keep (int64 indices in keep order)] : nmsp per image"""
        import torch
        from . import hip
        dev = hip.require_gpu()
        rows_list = [np.asarray(b, np.float32).reshape(-1, 5) for b in box_list]
        counts = np.array([len(r) for r in rows_list], np.int64)
        keeps = []
        for i0, i1 in self._chunks(counts * 44):
            t = time.perf_counter()
            rows, off = _stack(rows_list[i0:i1], 5, np.float32), _offsets(counts[i0:i1])
            total, I = len(rows), i1 - i0
            t = self._tick(timing, 'host', t)
            d_rows, d_off = _up(rows, dev), _up(off, dev)
            d_keep = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            d_nkeep = torch.empty(I, dtype=torch.int32, device=dev)
            need = int(hip.query('sn_prop_nms_workspace_bytes', total))
            if self._ws is None:
                self._ws = hip.Workspace()
            ws = self._ws.get(need)
            t = self._tick(timing, 'upload', t, sync=True)
            hip.call('sn_prop_nms', d_rows, d_off, I, int(counts[i0:i1].max(initial=0)), total, float(thresh), ws, need, d_keep, d_nkeep,
                     hip.stream())
            t = self._tick(timing, 'kernels', t, sync=True)
            keep, nkeep = d_keep.cpu().numpy(), d_nkeep.cpu().numpy()
            t = self._tick(timing, 'download', t)
            for k in range(I):
                keeps.append(keep[off[k]:off[k] + nkeep[k]].astype(np.int64))
            self._tick(timing, 'host', t)
        return keeps

    def assign(self, boxes_list, gt_boxes_list, gt_classes_list, names=None, timing=None):
        """per image (n,4) boxes, (g,4) ground truth, (g) classes -> per image (max_ov f32, max_cls i32, argmax i32)"""
        import torch
        from . import hip
        dev = hip.require_gpu()
        n = np.array([len(b) for b in boxes_list], np.int64)
        g = np.array([len(b) for b in gt_boxes_list], np.int64)
        self.check_gt(g, names)
        out = []
        for i0, i1 in self._chunks(n * 44 + g * 36):
            t = time.perf_counter()
            boxes, gt = _stack(boxes_list[i0:i1], 4, np.float64), _stack(gt_boxes_list[i0:i1], 4, np.float64)
            cls = _stack(gt_classes_list[i0:i1], 1, np.int32).reshape(-1)
            box_off, gt_off = _offsets(n[i0:i1]), _offsets(g[i0:i1])
            total, NG, I = len(boxes), len(gt), i1 - i0
            t = self._tick(timing, 'host', t)
            d = [_up(a, dev) for a in (boxes, box_off, gt, cls, gt_off)]
            d_ov = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            d_cls = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            d_arg = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            t = self._tick(timing, 'upload', t, sync=True)
            hip.call('sn_prop_assign', d[0], d[1], d[2], d[3], d[4], I, int(n[i0:i1].max(initial=0)), int(g[i0:i1].max(initial=0)), total,
                     NG, d_ov, d_cls, d_arg, hip.stream())
            t = self._tick(timing, 'kernels', t, sync=True)
            ov, mc, am = d_ov.cpu().numpy(), d_cls.cpu().numpy(), d_arg.cpu().numpy()
            t = self._tick(timing, 'download', t)
            for k in range(I):
                s = slice(box_off[k], box_off[k + 1])
                out.append((ov[s].copy(), mc[s].copy(), am[s].copy()))
            self._tick(timing, 'host', t)
        return out

    def recall(self, boxes_list, gt_boxes_list, gt_mask_list, A, thresholds, names=None, timing=None):
        """per image (n,4) boxes, (g,4) ground truth and (g) uint8 range masks -> (gt_ov, num_pos (A), hits (A,T)); gt_ov[a] is the
        list over the images WITH boxes of the reference's _gt_overlaps (float64, G_a values in round order, then zeros)"""
        import torch
        from . import hip
        dev = hip.require_gpu()
        thrs = np.ascontiguousarray(thresholds, np.float64).reshape(-1)
        if not 1 <= len(thrs) <= self.max_t:
            raise ValueError('evaluate_recall takes 1 to %d thresholds, got %d' % (self.max_t, len(thrs)))
        if not 1 <= A <= 8:
            raise ValueError('evaluate_recall takes 1 to 8 area ranges, got %d' % A)
        n = np.array([len(b) for b in boxes_list], np.int64)
        g = np.array([len(b) for b in gt_boxes_list], np.int64)
        self.check_gt(g, names)
        T = len(thrs)
        gt_ov = [[] for _ in range(A)]
        num_pos, hits = np.zeros(A, np.int64), np.zeros((A, T), np.int64)
        for i0, i1 in self._chunks(n * 36 + g * (37 + 8 * A)):
            t = time.perf_counter()
            boxes, gt = _stack(boxes_list[i0:i1], 4, np.float64), _stack(gt_boxes_list[i0:i1], 4, np.float64)
            mask = _stack(gt_mask_list[i0:i1], 1, np.uint8).reshape(-1)
            box_off, gt_off = _offsets(n[i0:i1]), _offsets(g[i0:i1])
            total, NG, I = len(boxes), len(gt), i1 - i0
            t = self._tick(timing, 'host', t)
            d = [_up(a, dev) for a in (boxes, box_off, gt, mask, gt_off, thrs)]
            d_ov = torch.empty(max(A * NG, 1), dtype=torch.float64, device=dev)
            d_pos = torch.empty(A, dtype=torch.int32, device=dev)
            d_hits = torch.empty(A * T, dtype=torch.int32, device=dev)
            t = self._tick(timing, 'upload', t, sync=True)
            hip.call('sn_prop_recall', d[0], d[1], d[2], d[3], d[4], d[5], I, A, T, int(g[i0:i1].max(initial=0)), total, NG, d_ov, d_pos,
                     d_hits, hip.stream())
            t = self._tick(timing, 'kernels', t, sync=True)
            ov = d_ov.cpu().numpy()[:A * NG].reshape(A, NG)
            num_pos += d_pos.cpu().numpy()
            hits += d_hits.cpu().numpy().reshape(A, T)
            t = self._tick(timing, 'download', t)
            for a in range(A):
                cs = np.concatenate(([0], np.cumsum((mask >> a) & 1, dtype=np.int64)))
                ga = cs[gt_off[1:]] - cs[gt_off[:-1]]              # G_a of every image
                for k in range(I):
                    if n[i0 + k] > 0:
                        gt_ov[a].append(ov[a, gt_off[k]:gt_off[k] + ga[k]].copy())
            self._tick(timing, 'host', t)
        return gt_ov, num_pos, hits


_EVALUATOR = None


def evaluator():
    global _EVALUATOR
    if _EVALUATOR is None:
        _EVALUATOR = ProposalRoidbEvaluator()
    return _EVALUATOR


def limits():
    return evaluator().limits()


# ---- arrays in, arrays out ------------------------------------------------------------------------------------------------------
def nms_proposals(box_list, thresh=0.7):
    """[(n,5) rows] -> [the rows nmsp keeps, in keep order]"""
    rows = [np.array(b) for b in box_list]
    keeps = evaluator().nms(rows, thresh)
    return [r[k] for r, k in zip(rows, keeps)]


def _proposal_records(box_list, gt_roidb, num_classes):
    if len(box_list) != len(gt_roidb):
        raise AssertionError('number of boxes matrix must match number of images')
    for i, b in enumerate(box_list):
        if b.ndim != 2 or b.shape[1] != 5:
            raise ValueError('image %d: proposals are (n,5) rows x1, y1, x2, y2, score, got %s' % (i, b.shape))
    has_gt = [rec['boxes'].size > 0 for rec in gt_roidb]
    empty = np.zeros((0, 4))
    res = evaluator().assign([b[:, :4] for b in box_list], [rec['boxes'] if h else empty for rec, h in zip(gt_roidb, has_gt)],
                             [rec['gt_classes'] if h else np.zeros(0, np.int32) for rec, h in zip(gt_roidb, has_gt)],
                             names=[rec.get('image') for rec in gt_roidb])
    roidb = []
    for i, (rec, b, (max_ov, max_cls, _)) in enumerate(zip(gt_roidb, box_list, res)):
        scores, boxes = b[:, -1], b[:, :4]
        num_boxes = boxes.shape[0]
        overlaps = np.zeros((num_boxes, num_classes), dtype=np.float32)
        pos = np.flatnonzero(max_ov > 0)           # (a float64 maximum that rounds to float32 zero writes a zero: nothing)
        overlaps[pos, max_cls[pos]] = max_ov[pos]
        roidb.append({'image': rec['image'], 'height': rec['height'], 'width': rec['width'], 'boxes': boxes,
                      'gt_classes': np.zeros((num_boxes,), dtype=np.int32), 'gt_overlaps': overlaps,
                      'max_classes': overlaps.argmax(axis=1), 'max_overlaps': overlaps.max(axis=1), 'flipped': False,
                      'proposal_scores': scores})
    return roidb


def merge_roidbs(a, b):
    """imdb.py:399-419, field by field, in place into `a`.  The reference's last condition tests the LISTS a and b for the key
    'proposal_scores' (`'proposal_scores' in a`), which is never true: b's scores are never appended, and a[i]['proposal_scores']
    keeps its own length.  Kept as it is (chip_worker does not read the field).  A roidb without the dense `gt_overlaps` (this
    project's ground-truth roidbs carry max_overlaps / max_classes only) merges to one without."""
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


def proposal_roidb(gt_roidb, box_list, num_classes, append_gt=True):
    """create_roidb_from_box_list (+ merge_roidbs into gt_roidb, in place, when append_gt) for callers that hold arrays"""
    rpn = _proposal_records([np.asarray(b) for b in box_list], gt_roidb, num_classes)
    return merge_roidbs(gt_roidb, rpn) if append_gt else rpn


def filter_roidb(roidb, config):
    """lib/data_utils/load_data.py:91-107: drop the images without a foreground or a background roi"""
    def is_valid(entry):
        ov = entry['max_overlaps']
        fg = np.where(ov >= config.TRAIN.FG_THRESH)[0]
        bg = np.where((ov < config.TRAIN.BG_THRESH_HI) & (ov >= config.TRAIN.BG_THRESH_LO + 0.0001))[0]
        return len(fg) > 0 or len(bg) > 0
    kept = [entry for entry in roidb if is_valid(entry)]
    print('filtered %d roidb entries: %d -> %d' % (len(roidb) - len(kept), len(roidb), len(kept)))
    return kept


# ---- recall ---------------------------------------------------------------------------------------------------------------------
class ProposalRecallResult(object):
    """area_counts (A-1): boxes per range (`all` excluded, as the reference counts);  num_pos (A);  hits (A,T);  recalls (A,T);
    ar (A);  gt_overlaps: per range the sorted overlap values;  thresholds;  summary(): the reference's all_log_info"""

    def __init__(self, area_names, area_counts, num_pos, hits, recalls, ar, gt_overlaps, thresholds, lines, timing=None):
        self.area_names, self.area_counts, self.num_pos, self.hits = area_names, area_counts, num_pos, hits
        self.recalls, self.ar, self.gt_overlaps, self.thresholds = recalls, ar, gt_overlaps, thresholds
        self.lines, self.timing = lines, timing

    def summary(self):
        return ''.join(self.lines)


def _areas(boxes):
    return (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)


def recall_inputs(roidb, candidate_boxes, area_ranges):
    """the host side of evaluate_recall's selection, in the arrays' own dtype as the reference computes it -> per image the boxes,
    the ground-truth rows (max_overlaps == 1: no crowd rows) and their uint8 range masks"""
    boxes_list, gt_list, mask_list = [], [], []
    for i, rec in enumerate(roidb):
        max_gt_overlaps = rec['gt_overlaps'].max(axis=1) if 'gt_overlaps' in rec else rec['max_overlaps']
        gt_inds = np.where((rec['gt_classes'] > 0) & (max_gt_overlaps == 1))[0]
        gt_boxes = rec['boxes'][gt_inds, :]
        gt_areas = _areas(gt_boxes)
        mask = np.zeros(len(gt_inds), np.uint8)
        for a, rng in enumerate(area_ranges):
            mask |= ((gt_areas >= rng[0]) & (gt_areas < rng[1])).astype(np.uint8) << a
        if candidate_boxes is None:
            boxes = rec['boxes'][np.where(rec['gt_classes'] == 0)[0], :]
        else:
            boxes = candidate_boxes[i]
        boxes_list.append(boxes)
        gt_list.append(gt_boxes)
        mask_list.append(mask)
    return boxes_list, gt_list, mask_list


def evaluate_recall(roidb, candidate_boxes=None, thresholds=None, area_names=None, area_ranges=None, timing=None):
    """imdb.py:291-396 -> ProposalRecallResult; the lines are printed as the reference prints them"""
    area_names = AREA_NAMES if area_names is None else list(area_names)
    area_ranges = AREA_RANGES if area_ranges is None else [list(r) for r in area_ranges]
    num_images = len(roidb)
    boxes_list, gt_list, mask_list = recall_inputs(roidb, candidate_boxes, area_ranges)
    lines = []

    def log(s):
        print(s)
        lines.append(s)
    area_counts = []
    for area_name, area_range in zip(area_names[1:], area_ranges[1:]):
        area_count = 0
        for boxes in boxes_list:
            boxes_areas = _areas(boxes)
            area_count += len(np.where((boxes_areas >= area_range[0]) & (boxes_areas < area_range[1]))[0])
        area_counts.append(area_count)
    total_counts = float(sum(area_counts))
    for area_name, area_count in zip(area_names[1:], area_counts):
        log('percentage of {} {}'.format(area_name, area_count / total_counts))
    log('average number of proposal {}'.format(total_counts / num_images))
    if thresholds is None:
        thresholds = np.arange(0.5, 0.95 + 1e-5, 0.05)
    A = len(area_ranges)
    gt_ov, num_pos, hits = evaluator().recall([np.asarray(b)[:, :4].astype(float) for b in boxes_list], [g.astype(float) for g in gt_list],
                                              mask_list, A, thresholds, names=[rec.get('image') for rec in roidb], timing=timing)
    all_recalls, all_ar, all_ov = [], [], []
    for a, area_name in enumerate(area_names):
        gt_overlaps = np.sort(np.hstack([np.zeros(0)] + gt_ov[a]))
        recalls = np.zeros_like(thresholds)
        with np.errstate(divide='ignore', invalid='ignore'):
            for i, t in enumerate(thresholds):
                recalls[i] = hits[a, i] / float(num_pos[a])        # numpy's division: nan (or inf) when the range has no row
        ar = recalls.mean()
        log('average recall for {}: {:.3f}'.format(area_name, ar))
        for threshold, recall in zip(thresholds, recalls):
            log('recall @{:.2f}: {:.3f}'.format(threshold, recall))
        all_recalls.append(recalls)
        all_ar.append(ar)
        all_ov.append(gt_overlaps)
    return ProposalRecallResult(area_names, np.array(area_counts, np.int64), num_pos, hits, np.array(all_recalls), np.array(all_ar), all_ov,
                                np.asarray(thresholds), lines, timing)


# ---- the reference's methods ------------------------------------------------------------------------------------------------------
def load_rpn_data(name, proposal_path='data/proposals', full=False):
    """imdb.py:81-118 -> (boxes, maps): the NMS'd rows per image; cached as [boxes, maps] in <name>_rpn_after_nms.pkl"""
    rpn_file = os.path.join(proposal_path, name + '_rpn.pkl')
    nms_cache_file = os.path.join(proposal_path, name + '_rpn_after_nms.pkl')
    if os.path.isfile(nms_cache_file):
        print('Reading cached proposals after ***NMS**** from {}'.format(nms_cache_file))
        with open(nms_cache_file, 'rb') as fh:
            [boxes, maps] = pickle.load(fh)
        print('Done!')
        return boxes, maps
    print('Loading {}....'.format(rpn_file))
    assert os.path.exists(rpn_file), 'rpn data not found at {}'.format(rpn_file)
    with open(rpn_file, 'rb') as fh:
        box_list = pickle.load(fh)
    print('Applying NMS...')
    boxes, maps = nms_proposals(box_list, 0.7), []
    print('Caching proposals after NMS to {}'.format(nms_cache_file))
    with open(nms_cache_file, 'wb') as fh:
        pickle.dump([boxes, maps], fh, pickle.HIGHEST_PROTOCOL)
    print('Done!')
    return boxes, maps


class ProposalRoidbMixin(object):
    """The reference's IMDB methods for an imdb object that has `name`, `num_classes` and `num_images`."""

    def load_rpn_data(self, proposal_path='data/proposals', full=False):
        return load_rpn_data(self.name, proposal_path, full)

    def create_roidb_from_box_list(self, box_list, mapping_list, gt_roidb):
        self.num_images = len(gt_roidb)
        return _proposal_records(box_list, gt_roidb, self.num_classes)

    def load_rpn_roidb(self, gt_roidb, proposal_path='proposals'):
        box_list, mapping_list = self.load_rpn_data(proposal_path)
        return self.create_roidb_from_box_list(box_list, mapping_list, gt_roidb)

    def rpn_roidb(self, gt_roidb, append_gt=False, cfg='', proposal_path='proposals'):
        self.cfg = cfg
        if append_gt:
            print('appending ground truth annotations')
            return merge_roidbs(gt_roidb, self.load_rpn_roidb(gt_roidb, proposal_path))
        return self.load_rpn_roidb(gt_roidb, proposal_path)     # (the reference drops proposal_path here: a TypeError there)

    merge_roidbs = staticmethod(merge_roidbs)

    def evaluate_recall(self, roidb, candidate_boxes=None, thresholds=None):
        assert len(roidb) == self.num_images
        return evaluate_recall(roidb, candidate_boxes, thresholds)
