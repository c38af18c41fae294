"""What the proposal-roidb tests and tests/golden/make_proproidb_golden.py share: the input sets (two hand-made, one seeded), the
loader of tests/golden/proproidb_v1.npz, the device's input layouts, the device run at the C ABI with guard bytes around every
operand, and seeded problems for the size seams.

A SET is dict(num_classes, gt_boxes [(g,4) f32], gt_classes [(g) i32], sizes [(width, height)], props [(n,5) f32 x1, y1, x2, y2,
score]).  Coordinates are multiples of a quarter pixel (the golden file stores them as int16 quarter pixels); scores are distinct
within an image in the golden sets: the reference's order of equal scores is undefined, so only such inputs have a reference
answer."""
import os

import numpy as np

from coco_eval_util import Guarded
from voc_eval_util import assert_same_bits, same_bits  # noqa: F401

import prop_roidb_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'proproidb_v1.npz')
SETS = ('small', 'edges', 'coco_like')
GOLDEN_KEYS = ('keep_idx', 'keep_counts', 'max_overlaps', 'max_classes', 'merged_rows', 'merged_scores', 'summary', 'summary_cand')


def _f32(rows, width):
    return np.array(rows, np.float32).reshape(-1, width)


def _pack(num_classes, images):
    """images: [(width, height, [(box, class)], [row5])]"""
    return {'num_classes': num_classes, 'sizes': [(w, h) for w, h, _, _ in images],
            'gt_boxes': [_f32([b for b, _ in g], 4) for _, _, g, _ in images],
            'gt_classes': [np.array([c for _, c in g], np.int32) for _, _, g, _ in images],
            'props': [_f32(p, 5) for _, _, _, p in images]}


def small_set():
    """four images that can be checked by hand, three classes"""
    return _pack(3, [
        # one 10 x 10 box; its copy, a copy shifted by one pixel (IoU 90 / 110: suppressed), a far box
        (100, 80, [([10, 10, 19, 19], 1)], [[10, 10, 19, 19, .9], [11, 10, 20, 19, .8], [60, 40, 79, 59, .7]]),
        # two boxes of two classes; the proposals overlap one each, the lower-scored one first in the file
        (120, 90, [([0, 0, 29, 29], 1), ([50, 20, 99, 69], 2)], [[52, 22, 99, 69, .3], [0, 0, 29, 24, .6], [0, 5, 29, 29, .5]]),
        # a chain a - b - c: b is suppressed by a, c overlaps only b and survives
        (200, 100, [([0, 0, 39, 39], 2)], [[0, 0, 39, 39, .95], [4, 0, 43, 39, .85], [12, 0, 51, 39, .75], [100, 50, 149, 89, .1]]),
        # a small box (24 x 24: range 0-25) and a large one (300 x 300: range 300-inf)
        (640, 480, [([100, 100, 123, 123], 1), ([200, 100, 499, 399], 2)],
         [[101, 101, 124, 124, .4], [190, 110, 489, 409, .8], [0, 0, 9, 9, .2]]),
    ])


def edges_set():
    """one case per image, four classes"""
    return _pack(4, [
        # 0: N == 0
        (100, 100, [([10, 10, 49, 49], 1)], []),
        # 1: G == 0
        (100, 100, [], [[10, 10, 49, 49, .5], [20, 20, 69, 69, .4]]),
        # 2: N < G (one box, three rows)
        (200, 200, [([0, 0, 49, 49], 1), ([100, 0, 149, 49], 2), ([0, 100, 49, 149], 3)], [[2, 2, 49, 49, .9]]),
        # 3: a proposal that overlaps no row, beside one that does
        (200, 200, [([0, 0, 49, 49], 1)], [[100, 100, 149, 149, .8], [0, 0, 49, 39, .7]]),
        # 4: two rows with an equal best overlap for one box (the box is their mirror axis): argmax names the first, and in the
        #    recall the lower row takes the box, the other row is left with the far box (overlap 0)
        (200, 200, [([0, 0, 19, 9], 1), ([0, 10, 19, 19], 2)], [[0, 5, 19, 14, .9], [150, 150, 169, 169, .8]]),
        # 5: two boxes with equal overlap on one row: the lower box index is the row's best
        (200, 200, [([10, 10, 29, 29], 3)], [[10, 10, 29, 24, .5], [10, 15, 29, 29, .6]]),
        # 6: a pair of proposals whose float32 IoU is exactly 7 / 10 (10 x 10 and its 10 x 7 part): `<=` keeps both
        (100, 100, [([60, 60, 89, 89], 1)], [[0, 0, 9, 9, .9], [0, 0, 9, 6, .8]]),
        # 7: a box / row pair whose float64 IoU is exactly 0.5: counted at the first threshold
        (100, 100, [([0, 0, 9, 9], 2)], [[0, 0, 9, 4, .9]]),
        # 8: a row of area exactly 25 ** 2: in 25-50, not in 0-25
        (100, 100, [([10, 10, 34, 34], 1)], [[10, 10, 34, 33, .9], [50, 50, 59, 59, .3]]),
    ])


def coco_like_set(n_images=24, seed=5):
    """81 classes; rows from synthetic.make_roidb; per image three `scales` of 60 .. 300 proposals stacked as
    imdb_proposal_extraction_wrapper stacks them: three fifths are copies of a row jittered by +-s of its size (s from 0.05, 0.15,
    0.3; a quarter of the rows are never copied, so that the recall stays below one), the rest uniform boxes"""
    from sniper_amd.synthetic import make_roidb
    rs = np.random.RandomState(seed)
    images = []
    for rec in make_roidb(n_images, seed=seed, num_classes=81):
        W, H = rec['width'], rec['height']
        gt = rec['boxes']
        found = np.flatnonzero(rs.rand(len(gt)) < 0.75)
        rows = []
        for _ in range(3):
            for _ in range(rs.randint(60, 301)):
                if len(found) and rs.rand() < 0.6:
                    b = gt[found[rs.randint(len(found))]]
                    s = (0.05, 0.15, 0.3)[rs.randint(3)]
                    w, h = b[2] - b[0] + 1, b[3] - b[1] + 1
                    x1, y1 = b[0] + rs.uniform(-s, s) * w, b[1] + rs.uniform(-s, s) * h
                    w, h = w * np.exp(rs.uniform(-s, s)), h * np.exp(rs.uniform(-s, s))
                else:
                    w, h = rs.uniform(8, 0.6 * W), rs.uniform(8, 0.6 * H)
                    x1, y1 = rs.uniform(0, W - 1 - w), rs.uniform(0, H - 1 - h)
                x1, y1 = np.clip(x1, 0, W - 2), np.clip(y1, 0, H - 2)
                x2, y2 = np.clip(x1 + w - 1, x1 + 1, W - 1), np.clip(y1 + h - 1, y1 + 1, H - 1)
                rows.append(list(np.round(np.array([x1, y1, x2, y2]) * 4) / 4) + [0.])
        rows = _f32(rows, 5)
        rows[:, 4] = ((rs.permutation(len(rows)) + 1.) / (len(rows) + 1.)).astype(np.float32)
        images.append((W, H, [(b, c) for b, c in zip(gt, rec['gt_classes'])], rows))
    return _pack(81, images)


def make_sets():
    return {'small': small_set(), 'edges': edges_set(), 'coco_like': coco_like_set()}


def gt_roidb_of(s):
    """the ground-truth roidb of a set, as a dataset's gt_roidb() returns it (dense one-hot gt_overlaps included)"""
    out = []
    for i, (boxes, cls, (w, h)) in enumerate(zip(s['gt_boxes'], s['gt_classes'], s['sizes'])):
        ov = np.zeros((len(cls), s['num_classes']), np.float32)
        ov[np.arange(len(cls)), cls] = 1.0
        out.append({'image': 'image_%06d.jpg' % i, 'height': h, 'width': w, 'boxes': boxes.copy(), 'gt_classes': cls.copy(),
                    'gt_overlaps': ov, 'max_classes': ov.argmax(axis=1), 'max_overlaps': ov.max(axis=1), 'flipped': False})
    return out


def _counts(arrays):
    return np.array([len(a) for a in arrays], np.int32)


def _cat(arrays, width, dtype):
    return np.concatenate([np.asarray(a, dtype).reshape(-1, width) for a in arrays] + [np.zeros((0, width), dtype)], axis=0)


def save_set(out, name, s):
    out['%s_num_classes' % name] = np.array(s['num_classes'], np.int32)
    out['%s_sizes' % name] = np.array(s['sizes'], np.int32).reshape(-1, 2)
    out['%s_gt_counts' % name], out['%s_prop_counts' % name] = _counts(s['gt_boxes']), _counts(s['props'])
    for key, arr in (('gt_q', _cat(s['gt_boxes'], 4, np.float32)), ('prop_q', _cat(s['props'], 5, np.float32)[:, :4])):
        q = np.round(arr * 4)
        assert (q / 4 == arr).all() and np.abs(q).max(initial=0) < 32768, 'coordinates are quarter pixels within int16'
        out['%s_%s' % (name, key)] = q.astype(np.int16)
    out['%s_gt_classes' % name] = _cat(s['gt_classes'], 1, np.int32).reshape(-1)
    out['%s_prop_scores' % name] = _cat(s['props'], 5, np.float32)[:, 4].copy()


def _split(arr, counts):
    return [a for a in np.split(arr, np.cumsum(counts)[:-1])] if len(counts) else []


_CACHE = {}


def load_golden():
    """{set: (SET, golden)}; golden: keep_idx / keep_counts (the rows load_rpn_data kept, as indices into the image's input rows),
    max_overlaps, max_classes (create_roidb_from_box_list, concatenated), merged_rows / merged_scores (per image the lengths of
    boxes and proposal_scores after merge_roidbs), summary / summary_cand (evaluate_recall's string on the merged roidb, without and
    with candidate_boxes = the kept rows) -- each written by the reference's own imdb.py"""
    if not _CACHE:
        z = np.load(GOLDEN)
        for name in SETS:
            g = lambda k: z['%s_%s' % (name, k)]
            gc, pc = g('gt_counts'), g('prop_counts')
            rows = np.concatenate((g('prop_q').astype(np.float32) / 4, g('prop_scores')[:, None]), axis=1).astype(np.float32)
            s = {'num_classes': int(g('num_classes')), 'sizes': [tuple(int(v) for v in r) for r in g('sizes')],
                 'gt_boxes': _split(g('gt_q').astype(np.float32) / 4, gc), 'gt_classes': _split(g('gt_classes'), gc),
                 'props': _split(rows, pc)}
            gold = {k: g(k) for k in GOLDEN_KEYS}
            for k in ('summary', 'summary_cand'):
                gold[k] = gold[k].tobytes().decode()
            _CACHE[name] = (s, gold)
    return _CACHE


# ---- the device's input layouts -----------------------------------------------------------------------------------------------------
def offsets(counts):
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int32)


def nms_layout(props):
    return {'rows': _cat(props, 5, np.float32), 'off': offsets(_counts(props))}


def assign_layout(boxes_list, gt_boxes, gt_classes):
    return {'boxes': _cat(boxes_list, 4, np.float64), 'box_off': offsets(_counts(boxes_list)), 'gt': _cat(gt_boxes, 4, np.float64),
            'gt_classes': _cat(gt_classes, 1, np.int32).reshape(-1), 'gt_off': offsets(_counts(gt_boxes))}


def area_masks(gt_boxes, area_ranges):
    """per image the uint8 range masks, the areas in the rows' own dtype"""
    out = []
    for b in gt_boxes:
        areas = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        m = np.zeros(len(b), np.uint8)
        for a, rng in enumerate(area_ranges):
            m |= ((areas >= rng[0]) & (areas < rng[1])).astype(np.uint8) << a
        out.append(m)
    return out


def recall_layout(boxes_list, gt_boxes, area_ranges):
    return {'boxes': _cat(boxes_list, 4, np.float64), 'box_off': offsets(_counts(boxes_list)), 'gt': _cat(gt_boxes, 4, np.float64),
            'gt_mask': _cat(area_masks(gt_boxes, area_ranges), 1, np.uint8).reshape(-1), 'gt_off': offsets(_counts(gt_boxes)),
            'A': len(area_ranges)}


def restatement(nms_in, assign_in, recall_in, thresholds, thresh=0.7):
    out = dict(R.nms_ref(nms_in['rows'], nms_in['off'], thresh))
    out.update(R.assign_ref(assign_in['boxes'], assign_in['box_off'], assign_in['gt'], assign_in['gt_classes'], assign_in['gt_off']))
    out.update(R.recall_ref(recall_in['boxes'], recall_in['box_off'], recall_in['gt'], recall_in['gt_mask'], recall_in['gt_off'],
                            recall_in['A'], thresholds))
    return out


DEVICE_KEYS = ('keep', 'nkeep', 'max_ov', 'max_cls', 'argmax', 'gt_ov', 'num_pos', 'hits')


def limits():
    import ctypes
    from sniper_amd._lib import lib
    out = (ctypes.c_int32 * 6)()
    lib().call('sn_prop_limits', out)
    return dict(zip(('max_gt', 'max_t', 'assign_block', 'recall_threads', 'nms_tile', 'sort_tile'), (int(v) for v in out)))


def device_run(nms_in, assign_in, recall_in, thresholds, thresh=0.7):
    """sn_prop_nms, sn_prop_assign and sn_prop_recall at the C ABI -> the arrays named in DEVICE_KEYS; every operand in a guarded
    buffer, the guards (and that no input changed) checked.  An image of assign_in without proposals keeps the fill of its (empty)
    slice, so the outputs compare whole."""
    import torch
    from sniper_amd import hip
    G = Guarded()
    thrs = np.asarray(thresholds, np.float64)
    out = {}
    # nms
    rows, off = nms_in['rows'], nms_in['off']
    total, I = len(rows), len(off) - 1
    need = int(hip.query('sn_prop_nms_workspace_bytes', total))
    assert need >= 28 * total
    d_rows, d_off, ws = G.put(rows), G.put(off), G.out((need,), np.uint8)
    keep, nkeep = G.out((total,), np.int32), G.out((I,), np.int32)
    hip.call('sn_prop_nms', d_rows, d_off, I, int(np.diff(off).max(initial=0)), total, float(thresh), ws, need, keep, nkeep, hip.stream())
    # assign
    a = assign_in
    n_a, ng_a, I_a = len(a['boxes']), len(a['gt']), len(a['box_off']) - 1
    d = [G.put(a[k]) for k in ('boxes', 'box_off', 'gt', 'gt_classes', 'gt_off')]
    max_ov, max_cls, argmax = G.out((n_a,), np.float32), G.out((n_a,), np.int32), G.out((n_a,), np.int32)
    hip.call('sn_prop_assign', d[0], d[1], d[2], d[3], d[4], I_a, int(np.diff(a['box_off']).max(initial=0)),
             int(np.diff(a['gt_off']).max(initial=0)), n_a, ng_a, max_ov, max_cls, argmax, hip.stream())
    # recall
    r = recall_in
    n_r, ng_r, I_r, A, T = len(r['boxes']), len(r['gt']), len(r['box_off']) - 1, r['A'], len(thrs)
    e = [G.put(r[k]) for k in ('boxes', 'box_off', 'gt', 'gt_mask', 'gt_off')] + [G.put(thrs)]
    gt_ov, num_pos, hits = G.out((A, ng_r), np.float64), G.out((A,), np.int32), G.out((A, T), np.int32)
    hip.call('sn_prop_recall', e[0], e[1], e[2], e[3], e[4], e[5], I_r, A, T, int(np.diff(r['gt_off']).max(initial=0)), n_r, ng_r, gt_ov,
             num_pos, hits, hip.stream())
    torch.cuda.synchronize()
    G.check()
    shapes = {'keep': (keep, (total,), np.int32), 'nkeep': (nkeep, (I,), np.int32), 'max_ov': (max_ov, (n_a,), np.float32),
              'max_cls': (max_cls, (n_a,), np.int32), 'argmax': (argmax, (n_a,), np.int32), 'gt_ov': (gt_ov, (A, ng_r), np.float64),
              'num_pos': (num_pos, (A,), np.int32), 'hits': (hits, (A, T), np.int32)}
    for k, (view, shape, dtype) in shapes.items():
        out[k] = Guarded.read(view, shape, dtype)
    return out


# ---- seeded problems --------------------------------------------------------------------------------------------------------------
def seam_problems(seed, pairs):
    """one image per (N, G) pair.  Rows and boxes lie on a coarse grid with sizes from a short list, so that equal overlaps are
    common (every tie rule is exercised at every size) and all seven area ranges are hit; scores are quantised to 1/16 (ties in the
    NMS order).  -> (props [(N,5) f32], gt_boxes [(G,4) f32], gt_classes [(G) i32])"""
    rng = np.random.RandomState(seed)
    sides = np.array([12, 24, 25, 40, 80, 150, 250, 320])
    props, gts, classes = [], [], []
    for N, G in pairs:
        def boxes(n):
            x, y = 16 * rng.randint(0, 24, n), 16 * rng.randint(0, 24, n)
            w, h = sides[rng.randint(len(sides), size=n)], sides[rng.randint(len(sides), size=n)]
            return np.stack((x, y, x + w - 1, y + h - 1), axis=1).astype(np.float32).reshape(-1, 4)
        g = boxes(G)
        p = boxes(N)
        if G and N:
            near = rng.rand(N) < 0.6
            src = g[rng.randint(G, size=N)]
            p[near] = src[near] + 4 * rng.randint(-2, 3, (int(near.sum()), 4)).astype(np.float32)
            p[:, 2:] = np.maximum(p[:, 2:], p[:, :2] + 3)
        s = (rng.randint(1, 17, N) / 16.0).astype(np.float32)
        props.append(np.concatenate((p, s[:, None]), axis=1).astype(np.float32).reshape(-1, 5))
        gts.append(g)
        classes.append(rng.randint(1, 81, G).astype(np.int32))
    return props, gts, classes
