"""Box voting (TEST.BBOX_VOTE, sniper_amd/csrc/box_vote.hip) on one val-sized synthetic pass -- 5 000 images, 80 classes, 2 000
pre-NMS rows per image drawn in clusters from a seed -- beside the stages it sits between.

    python tools/box_vote_bench.py [--images 5000] [--rows 2000] [--ref-images 0] [--reps 5] [--out profiles/box_vote_bench.txt]

Reported, the variants alternating in one process after a warm-up run, timed with device events (the download with a host clock
that ends in a synchronise):
  * the stages of the pass on the stacked rows: copy (the pre-NMS rows the voters are read from), sn_soft_nms_batch, sn_box_vote,
    sn_det_cap_per_image, download;
  * Tester.aggregate_device on the same rows with voting off and on, interleaved, with the spread between the blocks;
  * the numpy restatement (tests/box_vote_ref.py) on the first --ref-images images (0 = all) on this node, its output compared
    with the device's on the bits;
  * pairs per second and two bounds computed from the shapes: float64 operations over the vector float64 peak, bytes over the
    HBM bandwidth."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

NC = 80
PEAK_F64 = 78.6e12          # vector float64 operations per second, MI355X data sheet
PEAK_HBM = 8.0e12           # bytes per second, MI355X data sheet
OPS_REJECT = 5              # float64 operations of a pair the overlap rejects on its width: min, max, subtract, add, compare
OPS_VOTER = 32              # of a voting pair: width and height (8), the query's area (5), the intersection (1), the union (2), the
                            # divide (1), two compares (2), the threshold compare (1), five adds, four multiplies, the narrowing aside


def make_pass(n_images, n_rows, seed=0, objects=60):
    """-> rows (total, 5) float32 stacked by (image, class), sizes (n_images * 80,): per image `objects` objects (a class, a
    centre in a 1000 x 1000 field, sides uniform in 20 .. 300), every row a copy of one of them with each coordinate jittered by
    N(0, 0.04 x side) and a score uniform in [0.01, 1]"""
    rs = np.random.RandomState(seed)
    cls = rs.randint(0, NC, (n_images, objects))
    wh = rs.uniform(20, 300, (n_images, objects, 2))
    xy = rs.uniform(0, 1000, (n_images, objects, 2))
    pick = rs.randint(0, objects, (n_images, n_rows))
    img = np.repeat(np.arange(n_images), n_rows)
    p = pick.ravel()
    w = wh[img, p]
    jit = rs.normal(0.0, 0.04, (len(p), 4)) * np.hstack((w, w))
    rows = np.empty((len(p), 5), np.float32)
    rows[:, :2] = xy[img, p] + jit[:, :2]
    rows[:, 2:4] = xy[img, p] + w + jit[:, 2:]
    rows[:, 4] = rs.uniform(0.01, 1.0, len(p))
    key = img * NC + cls[img, p]
    order = np.argsort(key, kind='stable')
    return np.ascontiguousarray(rows[order]), np.bincount(key, minlength=n_images * NC).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--rows', type=int, default=2000)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = all')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--thresh', type=float, default=0.8)
    ap.add_argument('--method', default='ID')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'box_vote_bench.txt'))
    a = ap.parse_args()
    import torch
    import box_vote_ref as R
    from sniper_amd import config as cfgmod
    from sniper_amd import hip, inference
    from sniper_amd.ext import box_vote
    from sniper_amd.ext.cpu_nms import _soft_ws
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('box voting, %d images x %d classes x %d pre-NMS rows per image, thresh %g, scoring %s; card: %s (%s, %d CUs)' % (
        a.images, NC, a.rows, a.thresh, a.method, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    rows, sizes = make_pass(a.images, a.rows)
    P, total, max_n = len(sizes), int(sizes.sum()), int(sizes.max())
    off = np.zeros(P + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    dev = torch.device('cuda', 0)
    src, d_off = torch.from_numpy(rows).to(dev), torch.from_numpy(off).to(dev)
    work = torch.empty_like(src)
    cnt = torch.empty((P,), dtype=torch.int32, device=dev)
    lim = box_vote.limits()
    host = []
    for _ in range(3):                                     # the host's share of a voting call: the tile table and its upload
        c = time.perf_counter()
        tiles = box_vote.tile_table(sizes, lim['tile'])
        c1 = time.perf_counter()
        d_tiles = torch.from_numpy(tiles).to(dev)
        torch.cuda.synchronize()
        host.append((1e3 * (c1 - c), 1e3 * (time.perf_counter() - c1)))
    method = box_vote.method_id(a.method)
    ws = _soft_ws(max_n, total, dev)
    say('%d problems, %d rows (largest problem %d, mean of the non-empty ones %.1f), %d tiles of %d kept rows, LDS chunks of %d rows' % (
        P, total, max_n, sizes[sizes > 0].mean(), len(tiles), lim['tile'], lim['chunk']))

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def one_pass(vote):
        """-> {stage: ms}; the rows start from the same pre-NMS state every time"""
        work.copy_(src)
        torch.cuda.synchronize()
        t = {}
        e0 = ev()
        pre = work.clone() if vote else None
        e1 = ev()
        hip.call('sn_soft_nms_batch', work, d_off, P, max_n, total, 0.55, 0.3, 0.001, 2, ws, cnt, hip.stream())
        e2 = ev()
        if vote:
            hip.call('sn_box_vote', work, pre, d_off, cnt, d_tiles, len(tiles), P, float(a.thresh), method, hip.stream())
        e3 = ev()
        hip.call('sn_det_cap_per_image', work, d_off, cnt, a.images, NC, 100, hip.stream())
        e4 = ev()
        torch.cuda.synchronize()
        c = time.perf_counter()
        h, k = work.cpu().numpy(), cnt.cpu().numpy()
        t['download'] = 1e3 * (time.perf_counter() - c)
        t['copy'], t['soft-NMS'], t['vote'], t['cap'] = e0.elapsed_time(e1), e1.elapsed_time(e2), e2.elapsed_time(e3), e3.elapsed_time(e4)
        return t, h, k

    one_pass(True), one_pass(False)                       # warm-up: code objects, allocator
    runs = {False: [], True: []}
    for _ in range(a.reps):
        for vote in (False, True):
            t, h, k = one_pass(vote)
            runs[vote].append(t)
            if vote:
                voted, kept = h, k
    med = lambda v, s: float(np.median([r[s] for r in runs[v]]))
    lo = lambda v, s: float(np.min([r[s] for r in runs[v]]))
    hi = lambda v, s: float(np.max([r[s] for r in runs[v]]))
    say('stages of the pass, median of %d alternating runs (min .. max), ms:          voting off                 voting on' % a.reps)
    for s in ('copy', 'soft-NMS', 'vote', 'cap', 'download'):
        say('  %-10s %34s %26s' % (s, '%8.3f (%8.3f .. %8.3f)' % (med(False, s), lo(False, s), hi(False, s)),
                                  '%8.3f (%8.3f .. %8.3f)' % (med(True, s), lo(True, s), hi(True, s))))
    v_ms, n_ms = med(True, 'vote'), med(True, 'soft-NMS')
    say('host share of a voting call: the tile table from the pre-NMS sizes %.1f ms (numpy, one core), its upload %.2f ms (best of 3)' % (
        min(h[0] for h in host), min(h[1] for h in host)))
    say('the vote launch %.3f ms beside sn_soft_nms_batch on the same rows %.3f ms: %.2f x' % (v_ms, n_ms, v_ms / n_ms))

    # pairs and bounds from the shapes (the kept counts of the soft-NMS are part of the shape: it keeps nearly every row)
    work.copy_(src)
    hip.call('sn_soft_nms_batch', work, d_off, P, max_n, total, 0.55, 0.3, 0.001, 2, ws, cnt, hip.stream())
    n_t = cnt.cpu().numpy().astype(np.int64)
    pairs = int((n_t * sizes).sum())
    tiles_q = -(-n_t // lim['tile'])
    byts = int((tiles_q * sizes).sum()) * 20 + int(n_t.sum()) * 40 + len(tiles) * 8 + int((tiles_q > 0).sum()) * 12
    ops_lo, ops_hi = pairs * OPS_REJECT, pairs * OPS_VOTER
    t_f64_lo, t_f64_hi, t_hbm = ops_lo / PEAK_F64, ops_hi / PEAK_F64, byts / PEAK_HBM
    say('%d kept rows, %d (kept row, pre-NMS row) pairs: %.2f G pairs / s' % (int(n_t.sum()), pairs, pairs / (v_ms * 1e-3) / 1e9))
    say('bounds from the shapes: float64 %.1f .. %.1f M operations (every pair rejected on its width .. every pair a voter) over %.1f T/s '
        '= %.4f .. %.4f ms; %.1f MB over %.1f TB/s = %.4f ms; the %s bound binds, the launch takes %.0f x the larger lower bound' % (
            ops_lo / 1e6, ops_hi / 1e6, PEAK_F64 / 1e12, 1e3 * t_f64_lo, 1e3 * t_f64_hi, byts / 1e6, PEAK_HBM / 1e12, 1e3 * t_hbm,
            'float64' if t_f64_lo > t_hbm else 'HBM', v_ms * 1e-3 / max(t_f64_lo, t_hbm)))

    # Tester.aggregate_device on the same rows: one scale, one chip per image, no valid range
    class Imdb(object):
        num_classes, classes, name, result_path = NC + 1, None, 'synthetic', None
    big64 = src.double()
    lens = torch.from_numpy(sizes.reshape(a.images, NC).astype(np.int32)).to(dev)
    dets = inference._Detections([[[np.zeros((0, 5))] for _ in range(a.images)] for _ in range(NC + 1)])
    img_off = np.concatenate(([0], np.cumsum(sizes.reshape(a.images, NC).sum(1))))
    for i in range(a.images):
        dets.device_parts[(i, 0)] = (big64[img_off[i]:img_off[i + 1]], lens[i])
    testers = {}
    for vote in (False, True):
        cfg_v = cfgmod.res101_e2e()
        cfg_v.TEST.SCALES, cfg_v.TEST.VALID_RANGES, cfg_v.TEST.MAX_PER_IMAGE = ((512, 512),), ((-1, -1),), 100
        cfg_v.TEST.BBOX_VOTE, cfg_v.TEST.BBOX_VOTE_TH, cfg_v.TEST.BBOX_VOTE_SCORING = vote, a.thresh, a.method
        testers[vote] = inference.Tester(None, Imdb(), [{} for _ in range(a.images)], None, cfg=cfg_v, batch_size=1)
    agg = {False: [], True: []}
    for rep in range(a.reps + 1):
        for vote in (False, True):
            torch.cuda.synchronize()
            c = time.perf_counter()
            out = testers[vote].aggregate_device([dets])
            torch.cuda.synchronize()
            if rep:
                agg[vote].append(1e3 * (time.perf_counter() - c))
            if vote and rep == a.reps:
                got_q = [out[1 + q % NC][q // NC] for q in range(P)]
                assert all(g.tobytes() == voted[off[q]:off[q] + kept[q]].tobytes() for q, g in enumerate(got_q)), \
                    'Tester.aggregate_device and the staged pass differ'
    say('Tester.aggregate_device (count, scatter, soft-NMS, [vote], cap, download, the per-class views), %d interleaved blocks, ms: '
        'voting off %.1f (%.1f .. %.1f), voting on %.1f (%.1f .. %.1f): +%.1f ms' % (
            a.reps, np.median(agg[False]), min(agg[False]), max(agg[False]), np.median(agg[True]), min(agg[True]), max(agg[True]),
            np.median(agg[True]) - np.median(agg[False])))

    # the numpy restatement on the first images, compared on the bits
    n = min(a.ref_images, a.images) if a.ref_images > 0 else a.images
    q_n, r_n = n * NC, int(off[n * NC])
    work.copy_(src)
    hip.call('sn_soft_nms_batch', work, d_off, P, max_n, total, 0.55, 0.3, 0.001, 2, ws, cnt, hip.stream())
    top_h, cnt_h = work[:r_n].cpu().numpy(), cnt[:q_n].cpu().numpy()
    c = time.perf_counter()
    want = top_h.copy()
    for q in range(q_n):
        if cnt_h[q]:
            s = slice(off[q], off[q] + cnt_h[q])
            want[s] = R.box_vote_ref(top_h[s], rows[off[q]:off[q + 1]], a.thresh, a.method)
    t_ref = time.perf_counter() - c
    torch.cuda.synchronize()
    c = time.perf_counter()
    got = box_vote.box_vote_stacked(top_h, cnt_h, rows[:r_n], sizes[:q_n], a.thresh, a.method)
    t_dev = time.perf_counter() - c
    assert got.tobytes() == want.tobytes(), 'the device and the restatement differ'
    moved = int((got[:, :4] != top_h[:, :4]).any(1).sum())
    say('restatement (numpy overlaps, a Python loop over the voters, one core) on %s %d images: %.2f s%s; the device on the same rows, '
        'upload and download included: %.2f ms; outputs bit-identical (%d rows, %d of them moved by the vote)' % (
            'all' if n == a.images else 'the first', n, t_ref,
            '' if n == a.images else ' (linear in the images: about %.0f s for %d)' % (t_ref * a.images / n, a.images), 1e3 * t_dev, r_n, moved))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
