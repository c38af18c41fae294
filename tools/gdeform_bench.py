"""Grouped deformable convolution (csrc/gdeform.hip) at the ResNeXt-101 stage-4 launch shape of a 20-chip step -- x 20 x 32 x 32 x
2048, num_group 64, num_deformable_group 4, 3x3, pad 2, dilation 2 -- beside the kernels it replaces, in one process on one card:
the fused forward against sn_deform_im2col + sn_gconv_fwd (the column written, then contracted on the dilated twin), the fused
weight gradient against sn_deform_im2col + sn_gconv_wgrad, and sn_gdeform_dcol against sn_gconv_dgrad and torch's copy_ of the
755 MB column.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/gdeform_bench.py
    python tools/gdeform_bench.py --report DIR > profiles/gdeform_bench.txt
    python tools/gdeform_bench.py --step [chips (20)] [steps per block (10)] [rounds (3)]      # no profiler

Every call is followed by a one-element sn_ew_f32 fill; the report cuts the kernel trace at those markers and sums the kernels of
each call from their start / end timestamps.  Condition (the report's exit status): median fused forward <= median im2col + median
sn_gconv_fwd, median fused weight gradient <= median im2col + median sn_gconv_wgrad; no margin.

--step: wall time of the training step of config.resnext101_e2e_dcn beside config.resnext101_e2e, alternating blocks (reported,
not gated)."""
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, H, C, GROUPS, DG, PD = 20, 32, 2048, 64, 4, 2
REPS, WARM = 4, 1
CALLS = ['fwd fused', 'im2col', 'gconv fwd', 'wgrad fused', 'gconv wgrad', 'dcol', 'gconv dgrad', 'copy col']
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

    Cg, M, OC = C // GROUPS, N * H * H, 18 * DG
    x = torch.randn(N, H, H, C, device=d).half()
    dy = torch.randn(N, H, H, C, device=d).half()
    off = torch.randn(N, H, H, OC, device=d).half()            # offsets of about a pixel
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    w = (torch.randn(C, 9, Cg, device=d) * 0.1).half()
    dw = torch.zeros(C, 9, Cg, device=d)
    col, dcol = torch.empty(M, 9 * C, dtype=torch.float16, device=d), torch.empty(M, 9 * C, dtype=torch.float16, device=d)
    need_f = hip.query('sn_gdeform_wgrad_workspace_bytes', N, H, H, C, C, GROUPS, 3, 3, 1, PD, PD)
    need_g = hip.query('sn_gconv_wgrad_workspace_bytes', N, H, H, C, C, GROUPS, 3, 3, 1, PD, PD)
    ws = torch.empty(max(need_f, need_g, 256), dtype=torch.uint8, device=d)
    torch.cuda.synchronize()
    mark()
    for _ in range(REPS):
        hip.call('sn_gdeform_fwd', x, off, w, None, y, N, H, H, C, C, C, C, GROUPS, DG, 3, 3, 1, PD, PD, OC, 0, 0, st)
        mark()
        hip.call('sn_deform_im2col', x, off, col, N, H, H, C, 3, 3, 1, PD, PD, DG, OC, 0, st)
        mark()
        hip.call('sn_gconv_fwd', x, w, None, y, N, H, H, C, C, C, C, GROUPS, 3, 3, 1, PD, PD, 0, 0, st)
        mark()
        hip.call('sn_gdeform_wgrad', dy, x, off, dw, N, H, H, C, C, C, C, GROUPS, DG, 3, 3, 1, PD, PD, OC, 0, ws, need_f, st)
        mark()
        hip.call('sn_gconv_wgrad', dy, x, dw, N, H, H, C, C, C, C, GROUPS, 3, 3, 1, PD, PD, ws, need_g, st)
        mark()
        hip.call('sn_gdeform_dcol', dy, w, dcol, N, H, H, C, C, C, GROUPS, 3, 3, 1, PD, PD, st)
        mark()
        hip.call('sn_gconv_dgrad', dy, w, None, dx, N, H, H, C, C, C, C, C, GROUPS, 3, 3, 1, PD, PD, st)
        mark()
        dcol.copy_(col)
        mark()
    torch.cuda.synchronize()
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
    assert len(segs) == REPS * len(CALLS), (len(segs), REPS * len(CALLS))
    t = {c: [] for c in CALLS}
    for k, seg in enumerate(segs):
        rep, c = divmod(k, len(CALLS))
        assert seg, CALLS[c]
        if rep >= WARM:
            t[CALLS[c]].append(sum(e - s0 for s0, e, _ in seg) / 1e3)
    med = lambda v: sorted(v)[len(v) // 2]
    col_mb = N * H * H * 9 * C * 2 / 1e6
    print('grouped deformable 3x3 convolution, %d chips, x %d x %d x %d x %d (%.0f MB), num_group %d, num_deformable_group %d, pad = '
          'dilation = %d; column %.0f MB.  Kernel time per call in us, median (min - max) of %d repetitions after %d warm-up'
          % (N, N, H, H, C, N * H * H * C * 2 / 1e6, GROUPS, DG, PD, col_mb, REPS - WARM, WARM))
    for c in CALLS:
        print('  %-12s %8.1f (%.1f - %.1f)' % (c, med(t[c]), min(t[c]), max(t[c])))
    print('  copy col moves 2 x %.0f MB: %.2f TB/s; dcol writes %.0f MB: %.2f TB/s' % (col_mb, 2 * col_mb / med(t['copy col']), col_mb,
                                                                                      col_mb / med(t['dcol'])))
    ok = True
    for fused, parts in (('fwd fused', ('im2col', 'gconv fwd')), ('wgrad fused', ('im2col', 'gconv wgrad'))):
        a, b = med(t[fused]), sum(med(t[p]) for p in parts)
        good = a <= b
        ok = ok and good
        print('%-12s %8.1f us   %s %8.1f us   ratio %.2f   %s' % (fused, a, ' + '.join(parts), b, a / b, 'met' if good else 'NOT met'))
    print('dcol         %8.1f us   gconv dgrad %.1f us, copy col %.1f us (reported, not gated)'
          % (med(t['dcol']), med(t['gconv dgrad']), med(t['copy col'])))
    print('condition (each fused kernel no slower than the two kernels it replaces, medians): %s' % ('met' if ok else 'NOT met'))
    return 0 if ok else 1


def step(chips, steps, rounds):
    import torch
    from sniper_amd import config as cfgmod
    from sniper_amd.train import Trainer
    from tools.probes.frozen_bn_probe import card
    print('card: ' + card(), flush=True)
    trainers = [(name, Trainer(batch_images=chips, n_images=2 * chips, cfg=getattr(cfgmod, name)(chips)))
                for name in ('resnext101_e2e', 'resnext101_e2e_dcn')]
    for name, tr in trainers:
        for _ in range(3):
            tr.step()
            tr.next_batch()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in trainers}
    for _ in range(rounds):
        for name, tr in trainers:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step()
                tr.next_batch()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
    print('training step, %d chips, ms per step over blocks of %d steps, median (min - max) of %d alternating blocks' % (chips, steps, rounds))
    for name, _ in trainers:
        v = sorted(ms[name])
        print('  %-20s %7.2f (%.2f - %.2f)' % (name, v[len(v) // 2], v[0], v[-1]))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        sys.exit(report(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == '--step':
        a = [int(v) for v in sys.argv[2:]]
        step(*(a + [20, 10, 3][len(a):]))
    else:
        run()
