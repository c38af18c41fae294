"""The proposal roidb of one synthetic problem -- 5 000 images, 81 classes, three scales of up to 300 proposals stacked per image as
imdb_proposal_extraction_wrapper stacks them -- on the device (sniper_amd.proposal_roidb) and by the plain-numpy restatement of the
reference's imdb.py (tests/prop_roidb_ref.py) on the same node.

    python tools/prop_roidb_bench.py [--images 5000] [--props 900] [--ref-images 0] [--reps 3] [--out profiles/prop_roidb_bench.txt]

The device time is reported per call (NMS, assignment, recall) and in its stages: host (stacking the rows, the offsets, the
per-image results), upload (allocations and copies to the device), kernels, download.  evaluate_recall's own host work (the area
membership of every row in numpy, the strings) is in its total.  The restatement (the reference's per-image Python loops, one core,
without its Pool(32)) runs on the first --ref-images images (default: all; its cost is linear in the images and the line says when
it was scaled), and on those the device is compared as tests/test_gpu_prop_roidb.py compares: the kept rows, every array of the
merged roidb, num_pos, hits, the overlap values and the summary string, all on the bits."""
import argparse
import contextlib
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def make_problem(n_images, n_props, num_classes=81, seed=0):
    """the ground-truth roidb of synthetic.make_roidb; per image three scales of n_props / 6 .. n_props / 3 proposals: three fifths
    are copies of a box jittered by +-s of its size (s from 0.05, 0.15, 0.3; a quarter of the boxes are never copied), the rest
    uniform boxes; float32 rows on a quarter-pixel grid, distinct scores"""
    from sniper_amd import synthetic
    roidb = synthetic.make_roidb(n_images=n_images, seed=seed, num_classes=num_classes)
    rs = np.random.RandomState(seed + 1)
    box_list = []
    for r in roidb:
        W, H, gt = r['width'], r['height'], np.asarray(r['boxes'], np.float64)
        n = int(rs.randint(n_props // 6, n_props // 3 + 1, 3).sum())
        found = np.flatnonzero(rs.rand(len(gt)) < 0.75)
        w, h = rs.uniform(8, 0.6 * W, n), rs.uniform(8, 0.6 * H, n)
        x1, y1 = rs.uniform(0, W - 1 - w), rs.uniform(0, H - 1 - h)
        if len(found):
            near = rs.rand(n) < 0.6
            b = gt[found[rs.randint(len(found), size=n)]]
            s = rs.choice((0.05, 0.15, 0.3), size=n)
            bw, bh = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
            x1 = np.where(near, b[:, 0] + rs.uniform(-1, 1, n) * s * bw, x1)
            y1 = np.where(near, b[:, 1] + rs.uniform(-1, 1, n) * s * bh, y1)
            w = np.where(near, bw * np.exp(rs.uniform(-1, 1, n) * s), w)
            h = np.where(near, bh * np.exp(rs.uniform(-1, 1, n) * s), h)
        x1, y1 = np.clip(x1, 0, W - 2), np.clip(y1, 0, H - 2)
        x2, y2 = np.clip(x1 + w - 1, x1 + 1, W - 1), np.clip(y1 + h - 1, y1 + 1, H - 1)
        rows = np.round(np.stack((x1, y1, x2, y2, np.zeros(n)), axis=1) * 4) / 4
        rows[:, 4] = (rs.permutation(n) + 1.) / (n + 1.)
        box_list.append(rows.astype(np.float32))
    return roidb, box_list


def quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def same_roidb(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b), (i, sorted(a), sorted(b))
        for k in a:
            if isinstance(b[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (i, k)
            else:
                assert a[k] == b[k], (i, k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--props', type=int, default=900)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = all')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prop_roidb_bench.txt'))
    a = ap.parse_args()
    import torch
    from sniper_amd import proposal_roidb as P
    import prop_roidb_ref as R
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('proposal roidb, %d images x 81 classes x three scales of up to %d proposals; card: %s (%s, %d CUs)' % (
        a.images, a.props // 3, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    gt_roidb, box_list = make_problem(a.images, a.props)
    fresh = lambda n=None: [dict(r) for r in gt_roidb[:n]]
    ev = P.evaluator()
    runs = []
    for _ in range(a.reps + 1):                       # the first run warms the allocator and loads the code objects
        tn, ta, tr = {}, {}, {}
        t0 = time.perf_counter()
        keeps = ev.nms(box_list, 0.7, timing=tn)
        t1 = time.perf_counter()
        kept = [b[k] for b, k in zip(box_list, keeps)]
        ev.assign([b[:, :4] for b in kept], [r['boxes'] for r in gt_roidb], [r['gt_classes'] for r in gt_roidb], timing=ta)
        t2 = time.perf_counter()
        merged = quiet(P.proposal_roidb, fresh(), kept, 81)
        t3 = time.perf_counter()
        res = quiet(P.evaluate_recall, merged, timing=tr)
        t4 = time.perf_counter()
        runs.append({'nms': dict(tn, total=t1 - t0), 'assign': dict(ta, total=t2 - t1), 'roidb': {'total': t3 - t2},
                     'recall': dict(tr, total=t4 - t3)})
    med = lambda c, k: 1e3 * float(np.median([r[c].get(k, 0.0) for r in runs[1:]]))
    say('%d proposals, %d kept by the NMS, %d ground-truth boxes; AR (all) %.4f, recall@0.5 (all) %.4f' % (
        sum(len(b) for b in box_list), sum(len(k) for k in kept), sum(len(r['boxes']) for r in gt_roidb), res.ar[0], res.recalls[0][0]))
    for c, what in (('nms', 'load_rpn_data: sn_prop_nms (key, order, walk)'), ('assign', 'create_roidb_from_box_list: sn_prop_assign'),
                    ('recall', 'evaluate_recall: sn_prop_recall, 7 ranges x 10 thresholds')):
        say('  %-58s host %8.2f  upload %7.2f  kernels %8.2f  download %6.2f  call %9.2f ms  (first call %9.2f ms)' % (
            what, med(c, 'host'), med(c, 'upload'), med(c, 'kernels'), med(c, 'download'), med(c, 'total'), 1e3 * runs[0][c]['total']))
    say('  %-58s %9.2f ms  (assignment again + the dense rows + merge_roidbs, host)' % ('proposal_roidb(append_gt=True), the whole call',
                                                                                      med('roidb', 'total')))
    kernels = sum(med(c, 'kernels') for c in ('nms', 'assign', 'recall'))
    whole = med('nms', 'total') + med('roidb', 'total') + med('recall', 'total')
    say('kernels %.2f ms; pickle rows to merged roidb and recall, everything: %.2f ms (medians of %d runs)' % (kernels, whole, a.reps))
    # the restatement on the first images
    n = min(a.ref_images, a.images) if a.ref_images > 0 else a.images
    t = time.perf_counter()
    want_kept = R.load_rpn_data(box_list[:n])
    t_nms = time.perf_counter() - t
    t = time.perf_counter()
    want = R.merge_roidbs(fresh(n), R.create_roidb_from_box_list(want_kept, fresh(n), 81))
    t_roidb = time.perf_counter() - t
    t = time.perf_counter()
    want_rec = R.evaluate_recall(want)
    t_rec = time.perf_counter() - t
    t = time.perf_counter()
    got_kept = P.nms_proposals(box_list[:n])
    got = quiet(P.proposal_roidb, fresh(n), got_kept, 81)
    got_rec = quiet(P.evaluate_recall, got)
    t_dev = time.perf_counter() - t
    for x, y in zip(got_kept, want_kept):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    same_roidb(got, want)
    assert got_rec.summary() == want_rec['summary']
    assert np.array_equal(got_rec.num_pos, want_rec['num_pos']) and np.array_equal(got_rec.hits, want_rec['hits'])
    for x, y in zip(got_rec.gt_overlaps, want_rec['gt_overlaps']):
        assert x.tobytes() == y.tobytes()
    t_ref = t_nms + t_roidb + t_rec
    say('restatement (plain numpy, one core) on %s %d images: NMS %.2f s, roidb %.2f s, recall %.2f s = %.2f s%s;  the device path on the '
        'same images, host work included: %.2f ms = 1 / %.0f of it;  kept rows, every roidb array, num_pos, hits, the overlap values and '
        'the summary string bit-identical' % (
            'all' if n == a.images else 'the first', n, t_nms, t_roidb, t_rec, t_ref,
            '' if n == a.images else ' (linear in the images: scaled to %d images about %.0f s)' % (a.images, t_ref * a.images / n),
            1e3 * t_dev, t_ref / t_dev))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
