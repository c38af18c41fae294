"""COCO box evaluation of one val-sized synthetic problem -- 5 000 images, 80 classes, 100 detections per image -- on the device
(sniper_amd.evaluation) and by the plain-Python restatement of the reference's evaluator (tests/coco_eval_ref.py) on the same node.

    python tools/coco_eval_bench.py [--images 5000] [--dets 100] [--ref-images 0] [--reps 5] [--out profiles/coco_eval_bench.txt]

The device time is reported in its parts: host (the reference's rounding of the result rows and the CSR offsets, numpy), upload
(allocations and copies to the device), the two kernels (sn_coco_match, sn_coco_accumulate), the download of precision and recall.
The restatement (pure Python loops, like the reference's evaluate / accumulate) runs on the first --ref-images images (default: all;
its cost is linear in the images) and on those the device's precision and recall must equal it on the bits.  The share of an inference pass is stated
against 5 000 images at the README's 203 images/s = 24.6 s."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_problem(n_images, n_dets, num_classes=81, seed=0):
    """roidb of synthetic.make_roidb; per image n_dets detections: jittered copies of its boxes (three quarters) and random boxes,
    scores quantised to 1/1000"""
    from sniper_amd import synthetic
    roidb = synthetic.make_roidb(n_images=n_images, seed=seed, num_classes=num_classes)
    rs = np.random.RandomState(seed + 1)
    all_boxes = [[[] for _ in range(n_images)]] + [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(num_classes - 1)]
    for i, r in enumerate(roidb):
        gt = np.asarray(r['boxes'], np.float64)[np.asarray(r['gt_classes']) > 0]
        cls = np.asarray(r['gt_classes'])[np.asarray(r['gt_classes']) > 0]
        pick = rs.randint(len(gt), size=n_dets)
        b = gt[pick]
        wh = b[:, 2:] - b[:, :2] + 1
        s = rs.choice((0.03, 0.08, 0.2), size=(n_dets, 1))
        xy = b[:, :2] + rs.uniform(-1, 1, (n_dets, 2)) * s * wh
        wh = wh * np.exp(rs.uniform(-1, 1, (n_dets, 2)) * s)
        c = cls[pick].copy()
        rand = rs.rand(n_dets) < 0.25
        c[rand] = rs.randint(1, num_classes, rand.sum())
        xy[rand] = rs.uniform(0, 400, (rand.sum(), 2))
        wh[rand] = np.exp(rs.uniform(np.log(8), np.log(300), (rand.sum(), 2)))
        rows = np.hstack((xy, xy + wh - 1, np.round(rs.uniform(0.001, 1, (n_dets, 1)), 3))).astype(np.float32)
        for k in np.unique(c):
            all_boxes[k][i] = rows[c == k]
    return roidb, all_boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = all')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_eval_bench.txt'))
    a = ap.parse_args()
    import torch
    from sniper_amd.evaluation import COCOBoxEvaluator
    import coco_eval_ref as ref
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('COCO box evaluation, %d images x 80 classes x %d detections per image; card: %s (%s, %d CUs)' % (
        a.images, a.dets, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    roidb, all_boxes = make_problem(a.images, a.dets)
    ev = COCOBoxEvaluator.from_roidb(roidb, 81)
    runs = []
    for _ in range(a.reps + 1):                       # the first run warms the allocator and loads the code objects
        t = time.perf_counter()
        res = ev.evaluate(all_boxes)
        runs.append(dict(res.timing, total_s=time.perf_counter() - t))
    tm = res.timing
    say('%d problems, %d detections (%d kept), %d boxes; AP %.4f AP50 %.4f AR100 %.4f' % (
        tm['problems'], tm['detections'], tm['kept'], tm['boxes'], res.stats[0], res.stats[1], res.stats[8]))
    med = lambda k: float(np.median([r[k] for r in runs[1:]]))
    for k, what in (('host_s', 'host: result rows (rounding) + CSR offsets, numpy'), ('upload_s', 'upload: allocations + copies to the device'),
                    ('match_s', 'kernel sn_coco_match'), ('accumulate_s', 'kernels of sn_coco_accumulate'),
                    ('download_s', 'download of precision and recall'), ('total_s', 'evaluate(), everything')):
        say('  %-58s %9.2f ms  (first run %9.2f ms)' % (what, 1e3 * med(k), 1e3 * runs[0][k]))
    device_s = med('upload_s') + med('match_s') + med('accumulate_s') + med('download_s')
    infer_s = 5000 / 203.0
    say('device part (upload + kernels + download) %.2f ms = %.3f %% of a %.1f s inference pass (5 000 images at 203 images/s); '
        'with the host part %.2f ms = %.3f %%' % (1e3 * device_s, 100 * device_s / infer_s, infer_s, 1e3 * med('total_s'),
                                                   100 * med('total_s') / infer_s))
    # the restatement (= the reference's algorithm in Python) on the first images
    n = min(a.ref_images, a.images) if a.ref_images > 0 else a.images
    sub_boxes = [per[:n] for per in all_boxes]
    sub = COCOBoxEvaluator.from_roidb(roidb[:n], 81)
    rows, counts = sub.convert_detections(sub_boxes)
    kk, ii = np.nonzero(counts)
    dt = {'image': np.repeat(ii, counts[kk, ii]), 'category': np.repeat(kk, counts[kk, ii]), 'bbox': rows[:, :4], 'score': rows[:, 4], 'area': rows[:, 5]}
    gt = dict(sub.gt, iscrowd=sub.gt['iscrowd'].astype(np.int32), ignore=sub.gt['ignore'].astype(np.int32))
    t = time.perf_counter()
    e = ref.evaluate(gt, dt, 80)
    t_eval = time.perf_counter() - t
    t = time.perf_counter()
    precision, recall = ref.accumulate(e, 80)
    t_acc = time.perf_counter() - t
    got = sub.evaluate(sub_boxes)
    same = got.precision.tobytes() == precision.tobytes() and got.recall.tobytes() == recall.tobytes()
    say('restatement (plain Python, one core) on %s %d images: evaluate %.2f s + accumulate %.2f s = %.2f s%s;  the device on the same '
        'images: %.2f ms, precision and recall %s' % (
            'all' if n == a.images else 'the first', n, t_eval, t_acc, t_eval + t_acc,
            '' if n == a.images else ' (linear in the images: about %.0f s for %d)' % ((t_eval + t_acc) * a.images / n, a.images),
            1e3 * sum(got.timing[k] for k in ('host_s', 'upload_s', 'kernels_s', 'download_s')),
            'bit-identical' if same else 'DIFFER'))
    assert same
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
