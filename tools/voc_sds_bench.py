"""PASCAL VOC mask evaluation (voc_eval_sds) of one VOC-val-sized synthetic problem -- 1 449 images of up to 500 x 375, 20 classes, up to
100 detections per image with 28 x 28 maps -- on the device (sniper_amd.evaluation.VOCSegmEvaluator) and by the plain-Python restatement
of the reference's evaluator (tests/voc_sds_ref.py) on the same node.

    python tools/voc_sds_bench.py [--images 1449] [--dets 100] [--ref-images 0] [--reps 3] [--out profiles/voc_sds_bench.txt]

The device time is reported in its stages: host (rounding the boxes, the instance pool, the CSR offsets; numpy), upload (allocations
and copies to the device), sn_vocsds_mask_iou, sn_vocsds_match_iou, sn_voc_accumulate, the download of the APs.  The restatement (a
Python walk over every class's detections like the reference's, one resize and G array slices per detection) runs on the first
--ref-images images (0 = none; its cost is linear in the images), and on those the device is compared as tests/test_gpu_voc_sds.py
compares: dt_area, the overlaps, tp, fp, order, npos, rec, prec and the 11-point AP on the bits, the area AP within 2 * (n - 1) * 2^-53
for n recall changes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_problem(n_images, n_dets, K=20, M=28, seed=0):
    """-> (records, all_boxes, all_masks).  Per image 1 to 5 instances (ellipses or rectangles of 20 .. 300 pixels a side) and between
    n_dets / 2 and n_dets detections: three quarters are an instance's bound jittered (so that several claim one instance) with the
    instance's own pixels, sampled and quantised, as their map; the rest are random boxes of a random class with noise maps."""
    import voc_sds_util as U
    rng = np.random.RandomState(seed)
    records = []
    all_boxes = [[[] for _ in range(n_images)]] + [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(K)]
    all_masks = [[[] for _ in range(n_images)]] + [[np.zeros((0, M, M), np.float32) for _ in range(n_images)] for _ in range(K)]
    for i in range(n_images):
        h, w = (375, 500) if rng.rand() < 0.7 else (500, 375)
        h, w = h - rng.randint(0, 60), w - rng.randint(0, 60)
        rec, mine = [], []
        for _ in range(rng.randint(1, 6)):
            bh, bw = rng.randint(20, min(300, h)), rng.randint(20, min(300, w))
            y1, x1 = rng.randint(0, h - bh + 1), rng.randint(0, w - bw + 1)
            k, m = int(rng.randint(K)), U._blob(rng, bh, bw)
            rec.append({'mask': m, 'mask_bound': np.array([x1, y1, x1 + bw - 1, y1 + bh - 1]), 'mask_cls': k + 1})
            canvas = np.zeros((h, w), bool)
            canvas[y1:y1 + bh, x1:x1 + bw] = m
            mine.append((k, [x1, y1, x1 + bw - 1, y1 + bh - 1], canvas))
        records.append(rec)
        n = int(rng.randint(n_dets // 2, n_dets + 1))
        cls, rows, maps = [], [], []
        for _ in range(n):
            if rng.rand() < 0.75:
                k, g, canvas = mine[rng.randint(len(mine))]
                s = (0.05, 0.15, 0.3)[rng.randint(3)]
                gw, gh = g[2] - g[0] + 1, g[3] - g[1] + 1
                x, y = g[0] + rng.uniform(-s, s) * gw, g[1] + rng.uniform(-s, s) * gh
                bw, bh = gw * np.exp(rng.uniform(-s, s)), gh * np.exp(rng.uniform(-s, s))
                box = [x, y, x + bw - 1, y + bh - 1]
                m = U.map_of(canvas, box, M, rng)
            else:
                k = int(rng.randint(K))
                bw, bh = np.exp(rng.uniform(np.log(8), np.log(300), 2))
                x, y = rng.uniform(0, w - 8), rng.uniform(0, h - 8)
                box = [x, y, min(x + bw, w) - 1, min(y + bh, h) - 1]
                m = U.map_of(np.zeros((h, w), bool), box, M, rng, noise=0.5)
            cls.append(k)
            rows.append(box + [round(float(rng.uniform(0.001, 1)), 4)])
            maps.append(m)
        cls, rows, maps = np.array(cls), np.array(rows, np.float32), np.array(maps, np.float32)
        for k in np.unique(cls):
            all_boxes[k + 1][i], all_masks[k + 1][i] = rows[cls == k], maps[cls == k]
    return records, all_boxes, all_masks


def set_of(ev, all_boxes, all_masks):
    """the evaluator's inputs in the restatement's form"""
    boxes, scores, masks, counts = ev.convert_detections(all_boxes, all_masks)
    kk, ii = np.nonzero(counts)
    raw = np.concatenate([np.asarray(all_boxes[k + 1][i], np.float32).reshape(-1, 5) for k, i in zip(kk, ii)]) if len(kk) else np.zeros((0, 5), np.float32)
    dt = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'raw': raw, 'masks': masks}
    bits, pix_off = ev._pool(np.arange(len(ev.gt['image'])))
    gt = {'image': ev.gt['image'], 'category': ev.gt['category'], 'bound': ev.gt['bound'].astype(np.float64), 'bits': bits, 'pix_off': pix_off}
    return gt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=1449)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = the restatement is not run')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voc_sds_bench.txt'))
    a = ap.parse_args()
    import torch
    from sniper_amd.evaluation import VOC_CLASSES, VOCSegmEvaluator
    import voc_sds_ref as ref
    import voc_sds_util as U
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('PASCAL VOC mask evaluation (voc_eval_sds), %d images x 20 classes x up to %d detections per image, M = 28; card: %s (%s, %d CUs)' % (
        a.images, a.dets, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    t = time.perf_counter()
    records, all_boxes, all_masks = make_problem(a.images, a.dets)
    say('synthetic problem made in %.1f s' % (time.perf_counter() - t))
    ev = VOCSegmEvaluator(records, a.images, VOC_CLASSES)
    runs = []
    for _ in range(a.reps + 1):                       # the first run warms the allocator and loads the code objects
        t = time.perf_counter()
        res = ev.evaluate(all_boxes, all_masks)
        runs.append(dict(res.timing, total_s=time.perf_counter() - t))
    tm = res.timing
    say('%d problems, %d detections, %d instances, %d (detection, instance) pairs; Mean AP@0.5 %.4f Mean AP@0.7 %.4f' % (
        tm['problems'], tm['detections'], tm['instances'], tm['pairs'], res.mean_ap[0], res.mean_ap[1]))
    med = lambda k: float(np.median([r[k] for r in runs[1:]]))
    for k, what in (('host_s', 'host: rounding, instance pool, CSR offsets, numpy'), ('upload_s', 'upload: allocations + copies to the device'),
                    ('mask_iou_s', 'kernel sn_vocsds_mask_iou'), ('match_s', 'kernel sn_vocsds_match_iou'),
                    ('accumulate_s', 'kernels of sn_voc_accumulate'), ('download_s', 'download of the APs and npos'),
                    ('total_s', 'evaluate(), everything')):
        say('  %-56s %9.2f ms  (first run %9.2f ms)' % (what, 1e3 * med(k), 1e3 * runs[0][k]))
    say('kernels %.2f ms; device part (upload + kernels + download) %.2f ms; with the host part %.2f ms' % (
        1e3 * (med('mask_iou_s') + med('match_s') + med('accumulate_s')),
        1e3 * (med('upload_s') + med('mask_iou_s') + med('match_s') + med('accumulate_s') + med('download_s')), 1e3 * med('total_s')))
    n = min(a.ref_images, a.images)
    if n > 0:
        sub_boxes, sub_masks = [per[:n] for per in all_boxes], [per[:n] for per in all_masks]
        sub = VOCSegmEvaluator(records[:n], n, VOC_CLASSES)
        gt, dt = set_of(sub, sub_boxes, sub_masks)
        t = time.perf_counter()
        want = ref.run(gt, dt, 20)
        t_ref = time.perf_counter() - t
        t = time.perf_counter()
        got = sub.evaluate(sub_boxes, sub_masks, return_matches=True)
        t_dev = time.perf_counter() - t
        dev = dict(got.matches, ap07=got.ap07, npos=got.npos)
        U.assert_same_bits(dev, want, keys=('dt_box', 'dt_area', 'iou', 'dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det', 'order', 'npos', 'rec', 'prec', 'ap07'),
                           what='bench')
        n_terms = U.recall_changes(want['rec'], want['cls_off'])
        U.assert_area_within_bound(got.ap_area, want['ap_area'], n_terms, 'bench')
        say('restatement (plain Python, one core) on the first %d images, %d detections, %d pairs: %.2f s (linear in the images: about %.0f s '
            'for %d);  the device on the same images, matches read back: %.2f ms = 1 / %.0f of it;  dt_area, overlaps, tp, fp, order, npos, '
            'rec, prec, ap07 bit-identical, ap_area within its bound' % (
                n, len(dt['image']), len(want['iou']), t_ref, t_ref * a.images / n, a.images, 1e3 * t_dev, t_ref / t_dev))
    else:
        say('restatement not run (--ref-images 0)')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
