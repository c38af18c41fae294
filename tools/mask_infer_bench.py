"""The mask head's output stage at test time (csrc/mask_infer.hip) at its launch shapes -- N = 100 and N = 300
RoIs, HW = 28 x 28, C = 256, K = 80 -- in one process on one card: sn_mask_class_prob beside the launches of the stock chain it
replaces, as the engine issues them (mask_out's 1x1 convolution to 160 channels, pick x 2, the Concat's two copies, the relayout to
float32 (N, 2, HW) and the softmax), and beside torch's copy of the bytes of x (the traffic the fused kernel cannot avoid).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/mask_infer_bench.py
    python tools/mask_infer_bench.py --report DIR > profiles/mask_infer_bench.txt
    python tools/mask_infer_bench.py --step [images (8)] [rounds (3)]                  # no profiler

Every call is followed by a one-element sn_ew_f32 fill; the report cuts the kernel trace at those markers and sums the kernels of
each call from their start / end timestamps.  Nothing is gated in advance: the report states whether the fused kernel beats the
stock chain's summed kernel time at N = 100 -- the measurement that decides mask_inference.DEFAULT_FUSED -- and exits 0 either way.

--step: milliseconds per image of MaskTester.predict on a seeded synthetic roidb (100 boxes per image, one scale), fused and stock output
stage in alternating rounds (reported, not gated)."""
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = (100, 300)
HW, C, K = 28 * 28, 256, 80
REPS, WARM = 6, 1
CALLS = ['fused', 'stock chain', 'copy x']
MARK = 'ew_f32_kernel'


def run():
    import torch
    from sniper_amd import hip
    from tools.probes.frozen_bn_probe import card
    d = torch.device('cuda', 0)
    print('card: ' + card(), flush=True)
    flag = torch.zeros(1, device=d)
    st = hip.stream()

    def mark():
        hip.call('sn_ew_f32', None, None, flag, 1, 4, 1.0, st)

    torch.manual_seed(0)
    w = (torch.randn(2 * K, 1, C, device=d) * 0.05).half()
    bias = torch.randn(2 * K, device=d) * 0.5
    bufs = {}
    for N in SHAPES:
        x = torch.relu(torch.randn(N, HW, C, device=d)).half()          # random data, like mask_deconv_relu's output
        cls = torch.randint(0, K, (N,), device=d).float()
        bufs[N] = dict(x=x, cls=cls, cls_pos=cls + K, prob=torch.empty(N, HW, device=d), y=torch.empty(N, HW, 2 * K, dtype=torch.float16, device=d),
                       neg=torch.empty(N, HW, dtype=torch.float16, device=d), pos=torch.empty(N, HW, dtype=torch.float16, device=d),
                       both=torch.empty(N, HW, 2, dtype=torch.float16, device=d), z=torch.empty(N, 2, HW, device=d),
                       p=torch.empty(N, 2, HW, device=d), xc=torch.empty_like(x))
    torch.cuda.synchronize()
    mark()
    for N in SHAPES:
        b = bufs[N]
        for _ in range(REPS):
            hip.call('sn_mask_class_prob', b['x'], w, bias, b['cls'], b['prob'], N, HW, C, K, st)
            mark()
            hip.call('sn_conv_fwd', b['x'], w, bias, None, b['y'], N, 28, 28, C, C, 2 * K, 2 * K, 0, 1, 1, 1, 0, 1, 0, 0, st)
            hip.call('sn_pick_fwd', b['y'], b['cls_pos'], b['pos'], N, HW, 2 * K, st)
            hip.call('sn_pick_fwd', b['y'], b['cls'], b['neg'], N, HW, 2 * K, st)
            flat = b['both'].view(-1)
            hip.call('sn_copy2d', b['neg'], flat, N * HW, 1, 1, 2, 0, 0, st)
            hip.call('sn_copy2d', b['pos'], flat[1:], N * HW, 1, 1, 2, 0, 0, st)
            hip.call('sn_transpose_batched', b['both'], b['z'], N, HW, 2, HW * 2, 2 * HW, 2, HW, 0, 1, st)
            hip.call('sn_softmax_fwd', b['z'], b['p'], N, 2, HW, st)
            mark()
            b['xc'].copy_(b['x'])
            mark()
    torch.cuda.synchronize()
    for N in SHAPES:             # (after the last marker: torch's own kernels stay out of the timed segments)
        diff = (bufs[N]['prob'] - bufs[N]['p'][:, 1]).abs().max().item()
        print('N = %d: max |fused - stock chain| = %.3e (the stock chain rounds its logits to fp16)' % (N, diff), flush=True)
    print('done', flush=True)


def report(root):
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(files[0])))
    first = next(i for i, r in enumerate(rows) if MARK in r[2])
    segs, cur = [], []
    for s, e, name in rows[first + 1:]:
        if MARK in name:
            segs.append(cur)
            cur = []
        else:
            cur.append((s, e, name))
    assert len(segs) == len(SHAPES) * REPS * len(CALLS), (len(segs), len(SHAPES) * REPS * len(CALLS))
    med = lambda v: sorted(v)[len(v) // 2]
    print('mask head output stage, HW = %d, C = %d, K = %d.  Kernel time per call in us, median (min - max) of %d repetitions after %d '
          'warm-up; stock chain = sn_conv_fwd to %d channels + sn_pick_fwd x 2 + sn_copy2d x 2 (Concat) + sn_transpose_batched (to float32 '
          '(N, 2, HW)) + sn_softmax_fwd' % (HW, C, K, REPS - WARM, WARM, 2 * K))
    verdict = None
    for si, N in enumerate(SHAPES):
        t, parts = {c: [] for c in CALLS}, {}
        for k in range(REPS * len(CALLS)):
            rep, c = divmod(k, len(CALLS))
            seg = segs[si * REPS * len(CALLS) + k]
            assert seg, CALLS[c]
            if rep >= WARM:
                t[CALLS[c]].append(sum(e - s0 for s0, e, _ in seg) / 1e3)
                if CALLS[c] == 'stock chain':
                    for j, (s0, e, name) in enumerate(seg):
                        parts.setdefault((j, name.split('(')[0].split('<')[0][:40]), []).append((e - s0) / 1e3)
        x_mb = N * HW * C * 2 / 1e6
        print('N = %d (x %.1f MB)' % (N, x_mb))
        for c in CALLS:
            print('  %-12s %8.1f (%.1f - %.1f)' % (c, med(t[c]), min(t[c]), max(t[c])))
        for (j, name), v in sorted(parts.items()):
            print('      stock chain kernel %d  %-40s %8.1f' % (j, name, med(v)))
        f, s, cp = med(t['fused']), med(t['stock chain']), med(t['copy x'])
        print('  fused reads x at %.2f TB/s; copy x moves 2 x %.1f MB at %.2f TB/s; fused / stock chain = %.2f' % (
            x_mb / f, x_mb, 2 * x_mb / cp, f / s))
        if N == 100:
            verdict = f < s
    print('fused kernel beats the stock chain\'s summed kernel time at N = 100: %s -> the default of `fused` is %s' % (
        'yes' if verdict else 'NO', verdict))
    return 0


def step(images, rounds):
    import numpy as np
    import torch
    from sniper_amd import config as cfgmod
    from sniper_amd.mask_inference import MaskTester
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    from sniper_amd.synthetic import make_roidb
    from tools.probes.frozen_bn_probe import card
    print('card: ' + card(), flush=True)
    cfg = cfgmod.res101_e2e_mask(batch_images=1)
    rs = np.random.RandomState(0)
    roidb = make_roidb(images, seed=3, n_proposals=100)
    NC, R = 81, 100
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in roidb] for _ in range(NC)]
    for i, r in enumerate(roidb):
        r['image'] = rs.randint(0, 256, (r['height'], r['width'], 3)).astype(np.uint8)
        rows = r['boxes'][-100:]
        cls = rs.randint(1, NC, len(rows))
        for c in np.unique(cls):
            all_boxes[int(c)][i] = np.concatenate([rows[cls == c], rs.uniform(0, 1, (int((cls == c).sum()), 1))], 1).astype(np.float32)
    testers = [(f, MaskTester(mk.resnet_mx_101_e2e_mask(), cfg, None, None, rois_per_image=R, fused=f)) for f in (True, False)]
    for _, t in testers:
        for _ in range(2):               # bind every shape, capture the forwards
            t.predict(roidb, all_boxes)
    torch.cuda.synchronize()
    sec = {f: [] for f, _ in testers}
    for _ in range(rounds):
        for f, t in testers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t.predict(roidb, all_boxes)
            torch.cuda.synchronize()
            sec[f].append((time.perf_counter() - t0) / images)
    print('MaskTester.predict, %d synthetic images, 100 boxes each, scale %s, %d rows per pass: milliseconds per image, median (min - max) '
          'of %d alternating rounds; %d bound executors' % (images, testers[0][1].scale, R, rounds, testers[0][1].bound_executors()))
    for f, _ in testers:
        v = sorted(1e3 * s for s in sec[f])
        print('  fused=%-5s %8.3f (%.3f - %.3f)' % (f, v[len(v) // 2], v[0], v[-1]))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        sys.exit(report(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == '--step':
        a = [int(v) for v in sys.argv[2:]]
        step(*(a + [8, 3][len(a):]))
    else:
        run()
