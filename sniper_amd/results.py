"""Results files: what the reference's test run writes before it evaluates, and for a `test` image set the only thing it produces.

    write_coco_results('detections_val2014_results.json', all_boxes, image_ids, cat_ids)                  # coco.py:280-336, bbox
    write_coco_results(path, all_boxes, image_ids, cat_ids, 'segm', all_masks, image_sizes)               # ... segm
    result = evaluate_results_file(path, roidb, num_classes, 'segm')                                      # _do_python_eval
    write_voc_results('comp4_det_test_{:s}.txt', all_boxes, image_names, class_names)                     # pascal_voc.py:395-415

COCO (lib/dataset/coco.py:22-61, 264-336): `coco.evaluate_detections` writes detections_<set>_results.json -- one record per
detection, class-major, then image, then row -- and evaluates from that file.  A `segm` record carries the mask as compressed string
counts (pycocotools.mask.encode = rleEncode + rleToString); the strings of a whole file are coded in one pass on the device, and
decoded in one pass when a file is read back (sn_rle_string_len / sn_rle_to_string / sn_rle_string_count / sn_rle_from_string,
sniper_amd/csrc/rle_string.hip).  The records themselves -- rounding, order, layout -- are host work.

PASCAL VOC (lib/dataset/pascal_voc.py:395-415): one text file per class, host only.
"""
import json

import numpy as np

from .evaluation import (COCOBoxEvaluator, COCOSegmEvaluator, _cell_counts, _pool, paste_boxes, rle_counts, rle_from_string, rle_paste)

__all__ = ['rle_to_strings', 'rle_from_strings', 'coco_results', 'write_coco_results', 'load_coco_results', 'evaluate_results_file',
           'write_voc_results', 'rle_string_limits']

STATUS_OK, STATUS_OPEN, STATUS_FOREIGN, STATUS_LONG = 0, 1, 2, 3


def rle_string_limits():
    """sn_rle_string_limits -> dict: threads per workgroup, counts / characters per chunk, the most characters of a count; no device"""
    from . import hip
    out = np.zeros(3, np.int32)
    hip.call('sn_rle_string_limits', out)
    return dict(zip(('threads', 'chunk', 'max_chars'), (int(v) for v in out)))


def _off32(lengths, what):
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    if off[-1] >= 2 ** 31:
        raise ValueError('%s: %d in one call, 32-bit indexing takes fewer than 2^31' % (what, off[-1]))
    return off.astype(np.int32)


def _device_pool(a, dtype):
    """a host pool -> device tensor (one element where the pool is empty: the entry points take no NULL)"""
    import torch
    from . import hip
    return hip.dev(a) if len(a) else torch.zeros(1, dtype=dtype, device=hip.require_gpu())


def rle_to_strings(rles, timing=None):
    """rleToString (maskApi.c:181-193) of every mask in one pass on the device: rles = uint32 count arrays (or RLE dicts with such
    `counts`) -> list of str.  A difference of 2^29 or more takes seven characters (the reference allocates six and is undefined
    there).  One read-back between the two launches: the lengths."""
    import torch
    from . import hip
    rles = [np.asarray(r['counts'] if isinstance(r, dict) else r) for r in rles]
    N = len(rles)
    if N == 0:
        return []
    for n, r in enumerate(rles):
        if r.dtype == np.uint32 and r.ndim == 1:          # (what rle_paste and the decoders hand over: nothing to look at)
            continue
        if r.ndim != 1 or (r.size and (r.dtype.kind not in 'iu' or r.min() < 0 or r.max() > 0xFFFFFFFF)):
            raise ValueError('rle_to_strings: mask %d: counts are a flat array of non-negative integers below 2^32' % n)
    dev = hip.require_gpu()
    cnts, off = _pool(rles)
    run_off = _off32(np.diff(off), 'rle_to_strings: counts')
    total = int(run_off[-1])
    t0 = _clock(timing)
    d_c, d_roff = _device_pool(cnts.view(np.int32), torch.int32), hip.dev(run_off)
    d_len = torch.empty(N, dtype=torch.int32, device=dev)
    hip.call('sn_rle_string_len', d_c, d_roff, run_off, N, total, d_len, hip.stream())
    str_off = _off32(d_len.cpu().numpy().astype(np.int64), 'rle_to_strings: characters')
    chars = int(str_off[-1])
    d_s = torch.empty(max(chars, 1), dtype=torch.uint8, device=dev)
    hip.call('sn_rle_to_string', d_c, d_roff, run_off, hip.dev(str_off), str_off, N, total, chars, d_s, hip.stream())
    t1 = _clock(timing)
    text = d_s[:chars].cpu().numpy().tobytes().decode('ascii')
    so = str_off.tolist()                     # (Python ints: slicing with numpy scalars costs as much again as the slice)
    out = [text[so[n]:so[n + 1]] for n in range(N)]
    if timing is not None:
        timing.update(encode_s=t1 - t0, encode_download_s=_clock(timing) - t1, masks=N, runs=total, chars=chars)
    return out


def rle_from_strings(strings, timing=None):
    """rleFrString (maskApi.c:195-208) of every string in one pass on the device -> list of uint32 count arrays, what
    evaluation.rle_from_string gives for each.  ValueError names the first string that ends inside a count or holds a character
    outside chr(48) .. chr(111).  A count of more than seven characters -- legal input that no encoder produces -- is decoded on the
    host by evaluation.rle_from_string.  One read-back between the two launches: the counts and the status of every string."""
    import torch
    from . import hip
    N = len(strings)
    if N == 0:
        return []
    try:
        raw = [s if isinstance(s, bytes) else s.encode('latin-1') for s in strings]
    except (UnicodeEncodeError, AttributeError):
        bad = [n for n, s in enumerate(strings) if not isinstance(s, (str, bytes)) or any(ord(c) > 255 for c in s)][0]
        raise ValueError('rle_from_strings: string %d: a character outside chr(48) .. chr(111)' % bad)
    dev = hip.require_gpu()
    str_off = _off32([len(b) for b in raw], 'rle_from_strings: characters')
    chars = int(str_off[-1])
    pool = np.frombuffer(bytearray(b''.join(raw)), np.uint8)
    t0 = _clock(timing)
    d_s, d_soff = _device_pool(pool, torch.uint8), hip.dev(str_off)
    d_m, d_st = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    hip.call('sn_rle_string_count', d_s, d_soff, str_off, N, chars, d_m, d_st, hip.stream())
    m, status = d_m.cpu().numpy().astype(np.int64), d_st.cpu().numpy()
    for n in np.flatnonzero((status == STATUS_OPEN) | (status == STATUS_FOREIGN))[:1]:
        if status[n] == STATUS_OPEN:
            raise ValueError('rle_from_strings: string %d: rle_from_string: the string ends inside a count' % n)
        raise ValueError('rle_from_strings: string %d: a character outside chr(48) .. chr(111)' % n)
    m[status != STATUS_OK] = 0
    run_off = _off32(m, 'rle_from_strings: counts')
    total = int(run_off[-1])
    d_c = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    hip.call('sn_rle_from_string', d_s, d_soff, str_off, hip.dev(run_off), run_off, d_st, N, chars, total, d_c, hip.stream())
    t1 = _clock(timing)
    h_c = d_c[:total].cpu().numpy().view(np.uint32)
    ro = run_off.tolist()
    out = [h_c[ro[n]:ro[n + 1]] for n in range(N)]
    for n in np.flatnonzero(status == STATUS_LONG):
        out[n] = rle_from_string(raw[n])
    if timing is not None:
        timing.update(decode_s=t1 - t0, decode_download_s=_clock(timing) - t1, strings=N, runs=total, chars=chars,
                      host_fallback=int((status == STATUS_LONG).sum()))
    return out


def _clock(timing):
    if timing is None:
        return 0.
    import time
    import torch
    torch.cuda.synchronize()
    return time.perf_counter()


def _host(a):
    return np.asarray(a.cpu() if hasattr(a, 'cpu') else a)


def coco_results(all_boxes, image_ids, cat_ids, ann_type='bbox', all_masks=None, image_sizes=None, binary_thresh=0.4, timing=None):
    """The list `_write_coco_results` dumps (coco.py:22-61, 280-336): all_boxes[class][image] = (n,5) rows x1, y1, x2, y2, score (class
    0 = background) -> one dict per detection, class-major, then image, then row; empty cells leave nothing.
    bbox: 'bbox' = [x, y, w, h] with w = x2 - x1 + 1 in float64, rounded to 1 decimal, 'score' rounded to 8 -- the values of
      COCOBoxEvaluator.convert_detections, as Python floats.
    segm: 'segmentation' = {'size': [h, w], 'counts': str} and the score UNROUNDED (coco.py:57).  A cell of all_masks is the (n, M, M)
      probabilities of the cell's rows -- clip_boxes, paste_boxes, rle_paste at binary_thresh -- or a list of n RLE dicts, whose counts
      are coded as they are (string counts are passed through); image_sizes (I,2) = h, w.  All strings come from one rle_to_strings
      call."""
    plain = lambda ids: [int(v) if isinstance(v, np.integer) else v for v in ids]          # (json knows no numpy integers)
    image_ids, cat_ids = plain(image_ids), plain(cat_ids)
    K, I = len(cat_ids), len(image_ids)
    if ann_type == 'bbox':
        dt, counts = COCOBoxEvaluator({'image': [], 'category': [], 'bbox': [], 'area': [], 'iscrowd': []}, image_ids,
                                      cat_ids).convert_detections(all_boxes)
        kk, ii = np.nonzero(counts)
        img = np.repeat(np.asarray(image_ids, object)[ii], counts[kk, ii])
        cat = np.repeat(np.asarray(cat_ids, object)[kk], counts[kk, ii])
        boxes, scores = dt[:, :4].tolist(), dt[:, 4].tolist()
        return [{'image_id': img[n], 'category_id': cat[n], 'bbox': boxes[n], 'score': scores[n]} for n in range(len(dt))]
    if ann_type != 'segm':
        raise ValueError('coco_results: ann_type is \'bbox\' or \'segm\', got %r' % (ann_type,))
    if all_masks is None or image_sizes is None:
        raise ValueError('coco_results: segm records need all_masks and image_sizes')
    ev = COCOSegmEvaluator({'image': [], 'category': [], 'area': [], 'iscrowd': [], 'segmentation': []}, image_ids, cat_ids, image_sizes)
    counts = _cell_counts(all_boxes, K, I)
    if len(all_masks) != K + 1:
        raise ValueError('coco_results: all_masks[class][image]: %d classes (with the background) for %d categories' % (len(all_masks), K))
    recs, todo, where, pending = [], [], [], {}
    for k in range(K):
        if len(all_masks[k + 1]) != I:
            raise ValueError('coco_results: all_masks[%d] has %d images, all_boxes %d' % (k + 1, len(all_masks[k + 1]), I))
        for i in np.flatnonzero(counts[k]):
            rows, cell = _host(all_boxes[k + 1][i]).reshape(-1, 5).astype(np.float64), all_masks[k + 1][i]
            if len(cell) != len(rows):
                raise ValueError('coco_results: all_masks[%d][%d] has %d masks, all_boxes[%d][%d] %d rows' % (k + 1, i, len(cell), k + 1, i, len(rows)))
            h, w = (int(v) for v in ev.image_sizes[i])
            first = len(recs)
            recs.extend({'image_id': image_ids[i], 'category_id': cat_ids[k], 'segmentation': {'size': [h, w], 'counts': None},
                         'score': s} for s in rows[:, 4].tolist())
            if isinstance(cell, (list, tuple)):
                for n, seg in enumerate(cell):
                    what = 'coco_results: detection %d of all_masks[%d][%d]' % (n, k + 1, i)
                    if isinstance(seg, dict) and isinstance(seg.get('counts'), (str, bytes)):
                        if 'size' in seg and (int(seg['size'][0]), int(seg['size'][1])) != (h, w):
                            raise ValueError('%s: the mask is %d x %d, its image %d x %d' % (what, seg['size'][0], seg['size'][1], h, w))
                        c = seg['counts']
                        recs[first + n]['segmentation']['counts'] = c.decode('ascii') if isinstance(c, bytes) else c
                    else:
                        where.append(first + n), todo.append(rle_counts(seg, h, w, what))
                continue
            prob = _host(cell)
            if prob.ndim != 3 or prob.shape[1] != prob.shape[2]:
                raise ValueError('coco_results: all_masks[%d][%d] is neither a list of RLE dicts nor (n, M, M) probabilities' % (k + 1, i))
            slot = pending.setdefault(prob.shape[1], ([], [], [], []))
            slot[0].append(prob.astype(np.float32, copy=False)), slot[1].append(rows), slot[2].append((h, w, len(rows), k + 1, i))
            slot[3].extend(range(first, first + len(rows)))
    t0 = _clock(timing)
    for prob, rows, cells, at in pending.values():
        # clip_boxes and the rounding for all cells of one M at once (a call per cell costs more than everything else here); only a
        # refused box sends the cells through one by one, for the message that names the cell
        meta = np.asarray(cells, np.int64)
        hw = np.repeat(meta[:, :2], meta[:, 2], axis=0)
        try:
            box = paste_boxes(np.concatenate(rows), hw[:, :1], hw[:, 1:])
        except ValueError:
            for r, (h, w, _, k1, i) in zip(rows, cells):
                paste_boxes(r, h, w, 'coco_results: all_boxes[%d][%d]' % (k1, i))
            raise
        where.extend(at), todo.extend(rle_paste(np.concatenate(prob), box, hw, binary_thresh))
    if timing is not None:
        timing['paste_s'] = _clock(timing) - t0
    for n, s in zip(where, rle_to_strings(todo, timing)):
        recs[n]['segmentation']['counts'] = s
    return recs


def write_coco_results(path, all_boxes, image_ids, cat_ids, ann_type='bbox', all_masks=None, image_sizes=None, binary_thresh=0.4,
                       timing=None):
    """detections_<set>_results.json as the reference lays it out -- json.dump(results, f, sort_keys=True, indent=4) -- -> the number
    of records"""
    recs = coco_results(all_boxes, image_ids, cat_ids, ann_type, all_masks, image_sizes, binary_thresh, timing)
    import time
    t0 = time.perf_counter()
    with open(path, 'w') as f:
        json.dump(recs, f, sort_keys=True, indent=4)
    if timing is not None:
        timing['json_dump_s'] = time.perf_counter() - t0
    return len(recs)


def load_coco_results(path_or_list, image_ids, cat_ids, image_sizes=None, timing=None):
    """A results file (or its parsed list) -> (all_boxes, all_masks) in cell form, class 0 = background; all_masks is None for a bbox
    file.  bbox: rows [x, y, x + w - 1, y + h - 1, score] in float64.  segm: every string of the file is decoded in one
    rle_from_strings call; the cells are lists of {'size', 'counts': uint32 array}, the box columns are the mask's bounding box
    (rleToBbox, sn_rle_stats) as [x, y, x + w - 1, y + h - 1], zeros for an empty mask.  ValueError names the record with an unknown
    image or category id, or a mask whose size is not its image's."""
    if isinstance(path_or_list, (list, tuple)):
        recs = path_or_list
    else:
        with open(path_or_list) as f:
            recs = json.load(f)
    image_ids, cat_ids = list(image_ids), list(cat_ids)
    K, I = len(cat_ids), len(image_ids)
    img_of, cat_of = {v: n for n, v in enumerate(image_ids)}, {v: n for n, v in enumerate(cat_ids)}
    segm = bool(recs) and 'segmentation' in recs[0]
    if segm and image_sizes is None:
        raise ValueError('load_coco_results: a segm file needs image_sizes')
    sizes = np.asarray(image_sizes, np.int64).reshape(I, 2) if segm else None
    kk, ii = np.empty(len(recs), np.int64), np.empty(len(recs), np.int64)
    for n, r in enumerate(recs):
        if r.get('image_id') not in img_of:
            raise ValueError('load_coco_results: record %d: unknown image_id %r' % (n, r.get('image_id')))
        if r.get('category_id') not in cat_of:
            raise ValueError('load_coco_results: record %d: unknown category_id %r' % (n, r.get('category_id')))
        kk[n], ii[n] = cat_of[r['category_id']], img_of[r['image_id']]
        if segm:
            seg = r.get('segmentation')
            if not isinstance(seg, dict) or 'size' not in seg or not isinstance(seg.get('counts'), (str, bytes)):
                raise ValueError('load_coco_results: record %d: a segm record carries {\'size\', \'counts\': str}' % n)
            if (int(seg['size'][0]), int(seg['size'][1])) != (int(sizes[ii[n], 0]), int(sizes[ii[n], 1])):
                raise ValueError('load_coco_results: record %d: the mask is %d x %d, its image %d x %d' % (
                    n, seg['size'][0], seg['size'][1], sizes[ii[n], 0], sizes[ii[n], 1]))
        elif 'bbox' not in r:
            raise ValueError('load_coco_results: record %d: neither bbox nor segmentation' % n)
    order = np.argsort(kk * I + ii, kind='stable')             # cell by cell, file order inside a cell
    rows = np.zeros((len(recs), 5), np.float64)
    rows[:, 4] = [r['score'] for r in recs]
    rles = None
    if segm:
        rles = rle_from_strings([r['segmentation']['counts'] for r in recs], timing)
        if len(recs):
            t0 = _clock(timing)
            rows[:, :4] = _mask_boxes(rles, sizes[ii])
            if timing is not None:
                timing['bbox_s'] = _clock(timing) - t0
    elif len(recs):
        b = np.asarray([r['bbox'] for r in recs], np.float64).reshape(-1, 4)
        rows[:, 0], rows[:, 1] = b[:, 0], b[:, 1]
        rows[:, 2], rows[:, 3] = b[:, 0] + b[:, 2] - 1, b[:, 1] + b[:, 3] - 1
    all_boxes = [[np.zeros((0, 5), np.float64) for _ in range(I)] for _ in range(K + 1)]
    all_masks = [[[] for _ in range(I)] for _ in range(K + 1)] if segm else None
    key = (kk * I + ii)[order]
    cuts = np.flatnonzero(np.diff(key)) + 1 if len(key) else np.zeros(0, np.int64)
    for lo, hi in zip(np.concatenate([[0], cuts]).astype(np.int64), np.concatenate([cuts, [len(key)]]).astype(np.int64)):
        if hi == lo:
            continue
        sel = order[lo:hi]
        k, i = int(kk[sel[0]]), int(ii[sel[0]])
        all_boxes[k + 1][i] = rows[sel]
        if segm:
            size = [int(sizes[i, 0]), int(sizes[i, 1])]
            all_masks[k + 1][i] = [{'size': size, 'counts': rles[n]} for n in sel]
    return all_boxes, all_masks


def _mask_boxes(rles, hw):
    """rleToBbox of every mask on the device (sn_rle_stats) -> (N,4) float64 x1, y1, x2, y2 = x, y, x + w - 1, y + h - 1; an empty
    mask gives zeros"""
    import torch
    from . import hip
    dev = hip.require_gpu()
    N = len(rles)
    cnts, off = _pool(rles)
    hw = np.asarray(hw, np.int64).reshape(N, 2)
    rows = torch.empty((N, 6), dtype=torch.float64, device=dev)
    cum = torch.empty((max(int(off[-1]), 1), 2), dtype=torch.int32, device=dev)
    hip.call('sn_rle_stats', _device_pool(cnts.view(np.int32), torch.int32), hip.dev(_off32(np.diff(off), 'load_coco_results: counts')),
             hip.dev(hw.astype(np.int32)), None, N, int(off[-1]), int((hw[:, 0] * hw[:, 1]).max()), rows, cum, hip.stream())
    r = rows.cpu().numpy()
    out = np.zeros((N, 4), np.float64)
    some = (r[:, 2] > 0) & (r[:, 3] > 0)
    out[some, 0], out[some, 1] = r[some, 0], r[some, 1]
    out[some, 2], out[some, 3] = r[some, 0] + r[some, 2] - 1, r[some, 1] + r[some, 3] - 1
    return out


def evaluate_results_file(path, roidb, num_classes, ann_type='bbox'):
    """What `_do_python_eval` does with the file (coco.py:316-336): the records are loaded as COCO.loadRes loads them and evaluated
    against the roidb's ground truth -> COCOBoxResult | COCOSegmResult.  Image ids are 1.., category ids 1..num_classes-1, as the
    evaluators' from_roidb numbers them."""
    image_ids, cat_ids = range(1, len(roidb) + 1), range(1, num_classes)
    if ann_type == 'bbox':
        all_boxes, _ = load_coco_results(path, image_ids, cat_ids)
        return COCOBoxEvaluator.from_roidb(roidb, num_classes).evaluate(all_boxes)
    if ann_type != 'segm':
        raise ValueError('evaluate_results_file: ann_type is \'bbox\' or \'segm\', got %r' % (ann_type,))
    all_boxes, all_masks = load_coco_results(path, image_ids, cat_ids, [(r['height'], r['width']) for r in roidb])
    if all_masks is None:
        all_masks = [[[] for _ in roidb] for _ in range(num_classes)]
    return COCOSegmEvaluator.from_roidb(roidb, num_classes).evaluate(all_boxes, all_masks)


def write_voc_results(template, all_boxes, image_names, class_names):
    """write_pascal_results (pascal_voc.py:395-415): one file per class from template.format(cls), a line per detection -- image name,
    score to 3 decimals, the four coordinates + 1 (the VOCdevkit counts from 1) to 1 decimal; empty cells are skipped, a class
    without detections gets an empty file.  class_names excludes the background: all_boxes[k + 1] belongs to class_names[k].
    -> the number of lines.  Host only."""
    image_names, class_names = list(image_names), list(class_names)
    if len(all_boxes) != len(class_names) + 1:
        raise ValueError('write_voc_results: all_boxes[class][image]: %d classes (with the background) for %d class names' % (
            len(all_boxes), len(class_names)))
    lines = 0
    for k, cls in enumerate(class_names):
        if len(all_boxes[k + 1]) != len(image_names):
            raise ValueError('write_voc_results: all_boxes[%d] has %d images, image_names %d' % (k + 1, len(all_boxes[k + 1]), len(image_names)))
        with open(template.format(cls), 'wt') as f:
            for i, index in enumerate(image_names):
                dets = _host(all_boxes[k + 1][i])
                if len(dets) == 0:
                    continue
                for d in dets.reshape(-1, 5):
                    f.write('{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n'.format(index, d[-1], d[0] + 1, d[1] + 1, d[2] + 1, d[3] + 1))
                    lines += 1
    return lines
