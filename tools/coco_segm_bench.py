"""COCO mask evaluation of one val-sized synthetic problem -- 5 000 images of 480 x 640, 80 classes, 100 detections per image, every
mask run-length encoded -- on the device (sniper_amd.evaluation.COCOSegmEvaluator) and by the plain-Python restatement of the
reference's evaluator (tests/coco_segm_ref.py) on the same node.

    python tools/coco_segm_bench.py [--images 5000] [--dets 100] [--ref-images 0] [--reps 3] [--out profiles/coco_segm_bench.txt]

The device call is reported in its parts, each closed by a synchronise, medians of --reps runs after a warm-up: host (validation of
the counts, pools, CSR offsets, chunking: numpy and Python), upload (allocations + copies, all chunks), sn_rle_stats, sn_rle_iou,
sn_coco_match_iou, sn_coco_accumulate, download.  The restatement (pure Python walks, like the reference's C) runs on the first
--ref-images images (0 = all; its cost is linear in the images) and on those the device's IoU matrices, precision and recall must
equal it on the bits.  The masks of that problem are ellipses and rectangles written directly as runs.  The two conversion
stages are timed on their own after it: rle_from_polys on the polygons of synthetic.make_roidb(with_masks=True) for --images images,
and rle_paste on --paste-dets random 28 x 28 masks in those images' boxes (whole calls, host offsets and the read-back included);
a sample of each is bit-compared with the restatement."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, K = 480, 640, 80


def shape_runs(rs, cx, cy, rx, ry, ellipse):
    """counts of an ellipse or a rectangle (clipped to rows 1 .. H - 1 so that no run wraps into the next column)"""
    x0, x1 = max(0, int(np.ceil(cx - rx))), min(W - 1, int(np.floor(cx + rx)))
    if x1 < x0:
        x0 = x1 = min(W - 1, max(0, int(cx)))
    xs = np.arange(x0, x1 + 1)
    half = ry * np.sqrt(np.maximum(0., 1 - ((xs - cx) / rx) ** 2)) if ellipse else np.full(len(xs), ry)
    top = np.clip(np.floor(cy - half).astype(np.int64), 1, H - 2)
    bot = np.clip(np.ceil(cy + half).astype(np.int64), top + 1, H - 1)
    edges = np.stack((xs * H + top, xs * H + bot), axis=1).reshape(-1)
    return np.diff(np.concatenate([[0], edges, [H * W]])).astype(np.uint32)


def make_problem(n_images, n_dets, seed=0):
    """per image about 7 objects and n_dets detections: three quarters perturbed copies of its objects, the rest random shapes;
    scores quantised to 1/1000"""
    rs = np.random.RandomState(seed)
    gt = {k: [] for k in ('image', 'category', 'area', 'iscrowd', 'segmentation')}
    boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(K + 1)]
    masks = [[[] for _ in range(n_images)] for _ in range(K + 1)]
    seg = lambda c: {'size': [H, W], 'counts': c}
    for i in range(n_images):
        objs = []
        for _ in range(max(1, rs.poisson(7))):
            p = (rs.uniform(0, W), rs.uniform(0, H), np.exp(rs.uniform(np.log(4), np.log(150))), np.exp(rs.uniform(np.log(4), np.log(150))),
                 rs.rand() < 0.7)
            k = int(rs.randint(K))
            c = shape_runs(rs, *p)
            objs.append((p, k))
            gt['image'].append(i), gt['category'].append(k), gt['area'].append(float(c[1::2].sum())), gt['iscrowd'].append(int(rs.rand() < 0.05))
            gt['segmentation'].append(seg(c))
        cells = {}
        for _ in range(n_dets):
            if rs.rand() < 0.75:
                (cx, cy, rx, ry, e), k = objs[rs.randint(len(objs))]
                s = (0.03, 0.08, 0.2)[rs.randint(3)]
                p = (cx + rs.uniform(-s, s) * rx, cy + rs.uniform(-s, s) * ry, rx * np.exp(rs.uniform(-s, s)), ry * np.exp(rs.uniform(-s, s)), e)
            else:
                p = (rs.uniform(0, W), rs.uniform(0, H), np.exp(rs.uniform(np.log(4), np.log(150))), np.exp(rs.uniform(np.log(4), np.log(150))),
                     rs.rand() < 0.7)
                k = int(rs.randint(K))
            cells.setdefault(k, []).append((round(float(rs.uniform(0.001, 1)), 3), seg(shape_runs(rs, *p))))
        for k, rows in cells.items():
            boxes[k + 1][i] = np.array([[0, 0, 0, 0, s] for s, _ in rows], np.float64)
            masks[k + 1][i] = [m for _, m in rows]
    return gt, boxes, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = all')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--paste-dets', type=int, default=50000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_segm_bench.txt'))
    a = ap.parse_args()
    import torch
    from sniper_amd.evaluation import COCOSegmEvaluator
    import coco_segm_ref as ref
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('COCO mask evaluation, %d images of %d x %d x %d classes x %d detections per image, run-length encoded masks as input; card: %s (%s, %d CUs)' % (
            a.images, H, W, K, a.dets, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    t = time.perf_counter()
    gt, boxes, masks = make_problem(a.images, a.dets)
    say('problem made in %.1f s' % (time.perf_counter() - t))
    sizes = np.tile([[H, W]], (a.images, 1))
    t = time.perf_counter()
    ev = COCOSegmEvaluator(gt, range(a.images), range(K), sizes)
    say('evaluator built (the ground truth validated and kept as counts) in %.2f s' % (time.perf_counter() - t))
    runs = []
    for _ in range(a.reps + 1):                       # the first run warms the allocator and loads the code objects
        t = time.perf_counter()
        res = ev.evaluate(boxes, masks)
        runs.append(dict(res.timing, total_s=time.perf_counter() - t))
    tm = res.timing
    say('%d problems in %d chunks, %d detections (%d kept), %d annotations, %d runs, %d (detection, annotation) pairs; AP %.4f AP50 %.4f AR100 %.4f' % (
        tm['problems'], tm['chunks'], tm['detections'], tm['kept'], tm['boxes'], tm['runs'], tm['pairs'], res.stats[0], res.stats[1], res.stats[8]))
    med = lambda k: float(np.median([r[k] for r in runs[1:]]))
    for k, what in (('host_s', 'host: validation of the counts, pools, CSR offsets (Python + numpy)'),
                    ('upload_s', 'upload: allocations + copies to the device, all chunks'), ('stats_s', 'kernel sn_rle_stats, all chunks'),
                    ('iou_s', 'kernel sn_rle_iou, all chunks'), ('match_s', 'kernel sn_coco_match_iou, all chunks'),
                    ('accumulate_s', 'kernels of sn_coco_accumulate'), ('download_s', 'download of precision and recall'),
                    ('total_s', 'evaluate(), everything')):
        say('  %-72s %9.2f ms  (first run %9.2f ms)' % (what, 1e3 * med(k), 1e3 * runs[0][k]))
    device_s = sum(med(k) for k in ('upload_s', 'stats_s', 'iou_s', 'match_s', 'accumulate_s', 'download_s'))
    say('device part (upload + kernels + download) %.2f ms, the kernels alone %.2f ms; with the host part %.2f ms' % (
        1e3 * device_s, 1e3 * sum(med(k) for k in ('stats_s', 'iou_s', 'match_s', 'accumulate_s')), 1e3 * med('total_s')))
    # the restatement (= the reference's algorithm in Python) on the first images
    n = min(a.ref_images, a.images) if a.ref_images > 0 else a.images
    keep = np.flatnonzero(np.asarray(gt['image']) < n)
    sub_gt = {k: [gt[k][j] for j in keep] for k in gt}
    sub_boxes, sub_masks = [per[:n] for per in boxes], [per[:n] for per in masks]
    sub = COCOSegmEvaluator(sub_gt, range(n), range(K), sizes[:n])
    scores, rles, counts = sub.convert_detections(sub_boxes, sub_masks)
    kk, ii = np.nonzero(counts)
    r_dt = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'score': scores, 'rle': rles,
            'hw': np.tile([[H, W]], (len(rles), 1))}
    r_gt = {'image': sub.gt['image'], 'category': sub.gt['category'], 'area': sub.gt['area'], 'iscrowd': sub.gt['iscrowd'].astype(np.int32),
            'ignore': sub.gt['ignore'].astype(np.int32), 'rle': sub.gt_rle, 'hw': np.tile([[H, W]], (len(sub.gt_rle), 1))}
    t = time.perf_counter()
    want = ref.run(r_gt, r_dt, K, summary=False, cache={})
    t_ref = time.perf_counter() - t
    got = sub.evaluate(sub_boxes, sub_masks, return_matches=True)
    same = (got.precision.tobytes() == want['precision'].tobytes() and got.recall.tobytes() == want['recall'].tobytes() and
            got.matches['iou'].tobytes() == want['iou'].tobytes())
    say('restatement (plain Python, one core) on %s %d images: %.2f s%s;  the device on the same images: %.2f ms, IoU matrices, precision '
        'and recall %s' % ('all' if n == a.images else 'the first', n, t_ref,
                           '' if n == a.images else ' (linear in the images: about %.0f s for %d)' % (t_ref * a.images / n, a.images),
                           1e3 * sum(got.timing[k] for k in ('host_s', 'upload_s', 'kernels_s', 'download_s')),
                           'bit-identical' if same else 'DIFFER'))
    assert same
    # ---- the two conversion stages, whole calls ----
    from sniper_amd import synthetic
    from sniper_amd.evaluation import paste_boxes, rle_from_polys, rle_paste
    roidb = synthetic.make_roidb(n_images=a.images, seed=0, num_classes=81, with_masks=True)
    polys, phw, pbox = [], [], []
    for r in roidb:
        for j in np.flatnonzero(np.asarray(r['gt_classes']) > 0):
            polys.append(r['gt_masks'][j]), phw.append((r['height'], r['width'])), pbox.append(np.asarray(r['boxes'], np.float64)[j])
    phw = np.array(phw)
    ts = []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        got_p = rle_from_polys(polys, phw)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    m = min(len(polys), 300)
    t = time.perf_counter()
    want_p = [ref.rle_from_polys(polys[j], int(phw[j][0]), int(phw[j][1])) for j in range(m)]
    t_ref = time.perf_counter() - t
    same_p = all(np.array_equal(g, w_) for g, w_ in zip(got_p[:m], want_p))
    say('polygons: %d annotations, %d polygons, %d vertices, %d runs out; rle_from_polys %.1f ms (first run %.1f ms; host offsets, upload, '
        'sn_rle_poly_cross twice with the read-back, sn_rle_from_polys, download); restatement %.2f s for the first %d (about %.0f s for all); '
        'those %s' % (len(polys), sum(len(q) for q in polys), sum(len(v) for q in polys for v in q) // 2, sum(len(g) for g in got_p),
                      1e3 * float(np.median(ts[1:])), 1e3 * ts[0], t_ref, m, t_ref * len(polys) / m, 'bit-identical' if same_p else 'DIFFER'))
    rs = np.random.RandomState(7)
    nd = a.paste_dets
    pick = rs.randint(len(polys), size=nd)
    pm = rs.rand(nd, 28, 28).astype(np.float32)
    pb = np.concatenate([paste_boxes(pbox[j][None, :], phw[j][0], phw[j][1]) for j in pick])
    ts = []
    for _ in range(a.reps + 1):
        t = time.perf_counter()
        got_m = rle_paste(pm, pb, phw[pick], 0.4)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    m = min(nd, 40)
    t = time.perf_counter()
    want_m = [ref.paste(pm[j], pb[j], int(phw[pick[j]][0]), int(phw[pick[j]][1]), 0.4) for j in range(m)]
    t_ref = time.perf_counter() - t
    same_m = all(np.array_equal(g, w_) for g, w_ in zip(got_m[:m], want_m))
    say('paste (specified by this project, not pinned to OpenCV): %d masks of 28 x 28 into boxes of mean %.0f x %.0f, %d runs out; rle_paste '
        '%.1f ms (first run %.1f ms; upload of %.0f MB of masks, sn_rle_paste_count, the read-back, sn_rle_paste, download); restatement '
        '%.2f s for the first %d; those %s' % (nd, float((pb[:, 2] - pb[:, 0] + 1).mean()), float((pb[:, 3] - pb[:, 1] + 1).mean()),
                                               sum(len(g) for g in got_m), 1e3 * float(np.median(ts[1:])), 1e3 * ts[0], pm.nbytes / 1e6, t_ref, m,
                                               'bit-identical' if same_m else 'DIFFER'))
    assert same_p and same_m
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
