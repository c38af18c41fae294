"""PASCAL VOC box evaluation of one 2007_test-sized synthetic problem -- 4 952 images, 20 classes, up to 200 detections per image
(TEST.MAX_PER_IMAGE of the reference's VOC config) -- on the device (sniper_amd.evaluation.VOCBoxEvaluator) and by the plain-Python
restatement of the reference's evaluator (tests/voc_eval_ref.py) on the same node.

    python tools/voc_eval_bench.py [--images 4952] [--dets 200] [--ref-images 0] [--reps 5] [--out profiles/voc_eval_bench.txt]

The device time is reported in its parts: host (the rows of the result file -- v + 1 and the two roundings -- and the CSR offsets,
numpy), upload (allocations and copies to the device), the kernels (sn_voc_match, sn_voc_accumulate), the download of the APs.  The
restatement (a Python walk over every class's detections, like the reference's voc_eval, without the reference's detour through
result files on disk) runs on the first --ref-images images (default: all; its cost is linear in the images), and on those the
device is compared as tests/test_gpu_voc_eval.py compares: tp, fp, order, npos, rec, prec and the 11-point AP on the bits, the area AP
within 2 * (n - 1) * 2^-53 for n recall changes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_problem(n_images, n_dets, num_classes=21, seed=0):
    """roidb of synthetic.make_roidb with one box in ten difficult; per image between n_dets / 2 and n_dets detections: jittered copies
    of its boxes (three quarters, so that several claim one box) and random boxes, float32 rows, scores with 4 decimals (the
    rounding to 3 makes equal scores)"""
    from sniper_amd import synthetic
    roidb = synthetic.make_roidb(n_images=n_images, seed=seed, num_classes=num_classes)
    rs = np.random.RandomState(seed + 1)
    all_boxes = [[[] for _ in range(n_images)]] + [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(num_classes - 1)]
    for i, r in enumerate(roidb):
        fg = np.asarray(r['gt_classes']) > 0
        r['gt_difficult'] = (rs.rand(len(fg)) < 0.1).astype(np.int32)
        gt = np.asarray(r['boxes'], np.float64)[fg]
        cls = np.asarray(r['gt_classes'])[fg]
        n = int(rs.randint(n_dets // 2, n_dets + 1))
        pick = rs.randint(len(gt), size=n)
        b = gt[pick]
        wh = b[:, 2:] - b[:, :2] + 1
        s = rs.choice((0.03, 0.08, 0.2), size=(n, 1))
        xy = b[:, :2] + rs.uniform(-1, 1, (n, 2)) * s * wh
        wh = wh * np.exp(rs.uniform(-1, 1, (n, 2)) * s)
        c = cls[pick].copy()
        rand = rs.rand(n) < 0.25
        c[rand] = rs.randint(1, num_classes, rand.sum())
        xy[rand] = rs.uniform(0, 400, (rand.sum(), 2))
        wh[rand] = np.exp(rs.uniform(np.log(8), np.log(300), (rand.sum(), 2)))
        rows = np.hstack((xy, xy + wh - 1, np.round(rs.uniform(0.001, 1, (n, 1)), 4))).astype(np.float32)
        for k in np.unique(c):
            all_boxes[k][i] = rows[c == k]
    return roidb, all_boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=4952)
    ap.add_argument('--dets', type=int, default=200)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = all')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voc_eval_bench.txt'))
    a = ap.parse_args()
    import torch
    from sniper_amd.evaluation import VOCBoxEvaluator
    import voc_eval_ref as ref
    import voc_eval_util as U
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('PASCAL VOC box evaluation, %d images x 20 classes x up to %d detections per image; card: %s (%s, %d CUs)' % (
        a.images, a.dets, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    roidb, all_boxes = make_problem(a.images, a.dets)
    ev = VOCBoxEvaluator.from_roidb(roidb, 21)
    runs = []
    for _ in range(a.reps + 1):                       # the first run warms the allocator and loads the code objects
        t = time.perf_counter()
        res = ev.evaluate(all_boxes)
        runs.append(dict(res.timing, total_s=time.perf_counter() - t))
    tm = res.timing
    say('%d problems, %d detections, %d boxes (%d not difficult); Mean AP@0.5 %.4f Mean AP@0.7 %.4f (VOC07 metric)' % (
        tm['problems'], tm['detections'], tm['boxes'], int(res.npos.sum()), res.mean_ap[0], res.mean_ap[1]))
    med = lambda k: float(np.median([r[k] for r in runs[1:]]))
    for k, what in (('host_s', 'host: result rows (v + 1, rounding) + CSR offsets, numpy'), ('upload_s', 'upload: allocations + copies to the device'),
                    ('match_s', 'kernel sn_voc_match'), ('accumulate_s', 'kernels of sn_voc_accumulate'),
                    ('download_s', 'download of the APs and npos'), ('total_s', 'evaluate(), everything')):
        say('  %-62s %9.2f ms  (first run %9.2f ms)' % (what, 1e3 * med(k), 1e3 * runs[0][k]))
    device_s = med('upload_s') + med('match_s') + med('accumulate_s') + med('download_s')
    say('device part (upload + kernels + download) %.2f ms; with the host part %.2f ms' % (1e3 * device_s, 1e3 * med('total_s')))
    # the restatement (= the reference's algorithm in Python, stable sort) on the first images
    n = min(a.ref_images, a.images) if a.ref_images > 0 else a.images
    sub_boxes = [per[:n] for per in all_boxes]
    sub = VOCBoxEvaluator.from_roidb(roidb[:n], 21)
    t = time.perf_counter()
    rows, counts = sub.convert_detections(sub_boxes)
    t_rows = time.perf_counter() - t
    kk, ii = np.nonzero(counts)
    dt = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'rows': rows}
    gt = dict(sub.gt, difficult=sub.gt['difficult'].astype(np.int32))
    t = time.perf_counter()
    want = ref.run(gt, dt, 20)
    t_ref = time.perf_counter() - t
    t = time.perf_counter()
    got = sub.evaluate(sub_boxes, return_curves=True)
    t_dev = time.perf_counter() - t
    dev = dict(got.curves, ap07=got.ap07, npos=got.npos)
    U.assert_same_bits(dev, want, keys=('dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det', 'order', 'npos', 'rec', 'prec', 'ap07'), what='bench')
    n_terms = U.recall_changes(want['rec'], want['cls_off'])
    U.assert_area_within_bound(got.ap_area, want['ap_area'], n_terms, 'bench')
    ok = ~np.isnan(want['ap_area'])
    say('restatement (plain Python, one core, rows given) on %s %d images, %d detections: %.2f s%s;  the device on the same images, rows and '
        'curves included: %.2f ms = 1 / %.0f of it (%.2f ms without the %.2f ms of host rows: 1 / %.0f);  tp, fp, order, npos, rec, prec, '
        'ap07 bit-identical, ap_area within %.1e of it (bound %.1e)' % (
            'all' if n == a.images else 'the first', n, len(rows), t_ref,
            '' if n == a.images else ' (linear in the images: about %.0f s for %d)' % (t_ref * a.images / n, a.images),
            1e3 * t_dev, t_ref / t_dev, 1e3 * (t_dev - t_rows), 1e3 * t_rows, t_ref / max(t_dev - t_rows, 1e-9),
            float(np.abs(got.ap_area[ok] - want['ap_area'][ok]).max()), float((2.0 * (n_terms[ok] - 1) * 2.0 ** -53).min())))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
