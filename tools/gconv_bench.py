"""Grouped convolution (csrc/gconv.hip) at the ResNeXt-101 64x4d launch shapes of a 20-chip step -- stages 1 - 4 and the stride-2
openers of stages 2 and 3 -- forward, data gradient and weight gradient, each beside two yardsticks measured in the same process on
the same card: the DENSE kernels on a layer of the same C, O and geometry (sn_conv_fwd / sn_conv_dgrad / the batched weight
gradient: the same activation bytes, `groups` times the FLOPs -- the only way to run such a width without gconv.hip), and torch's
device copy of the same activation bytes.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/gconv_bench.py
    python tools/gconv_bench.py --report DIR > profiles/gconv_bench.txt

Every call is followed by a one-element sn_ew_f32 fill; the report cuts the kernel trace at those markers and sums the kernels of
each call from their start / end timestamps.  Condition (the report's last column and its exit status): every grouped kernel is
faster than its dense counterpart at every shape -- the slowest grouped repetition against the fastest dense one."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, GROUPS = 20, 64
# (name, C = O, H = W of the input, stride, pad = dil)
SHAPES = [('stage1', 256, 128, 1, 1), ('stage2 opener', 512, 128, 2, 1), ('stage2', 512, 64, 1, 1), ('stage3 opener', 1024, 64, 2, 1),
          ('stage3', 1024, 32, 1, 1), ('stage4 dil 2', 2048, 32, 1, 2)]
REPS, WARM = 4, 1
CALLS = ['fwd grouped', 'fwd dense', 'dgrad grouped', 'dgrad dense', 'wgrad grouped', 'wgrad dense', 'copy fwd', 'copy wgrad']
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

    for name, C, H, s, pd in SHAPES:
        Cg = C // GROUPS
        Ho = (H + 2 * pd - 2 * pd - 1) // s + 1
        x = torch.randn(N, H, H, C, device=d).half()
        dy = torch.randn(N, Ho, Ho, C, device=d).half()
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        wg = (torch.randn(C, 9, Cg, device=d) * 0.1).half()
        wd = (torch.randn(C, 9, C, device=d) * 0.02).half()
        wdT = (torch.randn(C, 9, C, device=d) * 0.02).half()
        dwg, dwd = torch.zeros(C, 9, Cg, device=d), torch.zeros(C, 9, C, device=d)
        need_g = hip.query('sn_gconv_wgrad_workspace_bytes', N, H, H, C, C, GROUPS, 3, 3, s, pd, pd)
        tab = hip.wgrad_table([(dy, x, dwd, N, H, H, C, C, C, C, 3, 3, s, pd, pd)])
        need_d = hip.query('sn_conv_wgrad_batch_workspace_bytes', tab, 1)
        ws = torch.empty(max(need_g, need_d, 256), dtype=torch.uint8, device=d)
        half = (x.numel() + dy.numel()) // 2          # a copy of `half` elements reads + writes the bytes of x and y together
        ca, cb = torch.randn(half, device=d).half(), torch.empty(half, dtype=torch.float16, device=d)
        torch.cuda.synchronize()
        mark()
        for _ in range(REPS):
            hip.call('sn_gconv_fwd', x, wg, None, y, N, H, H, C, C, C, C, GROUPS, 3, 3, s, pd, pd, 0, 0, st)
            mark()
            hip.call('sn_conv_fwd', x, wd, None, None, y, N, H, H, C, C, C, C, 0, 3, 3, s, pd, pd, 0, 0, st)
            mark()
            hip.call('sn_gconv_dgrad', dy, wg, None, dx, N, H, H, C, C, C, C, C, GROUPS, 3, 3, s, pd, pd, st)
            mark()
            hip.call('sn_conv_dgrad', dy, wdT, None, dx, N, H, H, C, C, C, C, C, 3, 3, s, pd, pd, 0, st)
            mark()
            hip.call('sn_gconv_wgrad', dy, x, dwg, N, H, H, C, C, C, C, GROUPS, 3, 3, s, pd, pd, ws, need_g, st)
            mark()
            hip.call('sn_conv_wgrad_batch', tab, 1, ws if need_d else None, need_d, st)
            mark()
            cb.copy_(ca)
            mark()
            cb.copy_(ca)
            mark()
        torch.cuda.synchronize()
        print('%s done' % name, flush=True)
        del x, dy, y, dx, wd, wdT, dwd, ws, ca, cb
        torch.cuda.empty_cache()


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
    # per shape: the opening marker closes a segment of set-up kernels (allocation fills, randn), then REPS x CALLS segments
    per = REPS * len(CALLS)
    assert len(segs) == len(SHAPES) * per + len(SHAPES) - 1, (len(segs), len(SHAPES) * per)
    print('grouped 3x3 convolution, %d chips, num_group %d: kernel time per call in us, median (min - max) of %d repetitions after %d '
          'warm-up; dense = the same C, O and geometry on sn_conv_fwd / sn_conv_dgrad / sn_conv_wgrad_batch; copy = torch copy_ of the '
          'same activation bytes (x + y)' % (N, GROUPS, REPS - WARM, WARM))
    ok, k = True, 0
    med = lambda v: sorted(v)[len(v) // 2]
    for i, (name, C, H, s, pd) in enumerate(SHAPES):
        if i:
            k += 1                      # set-up kernels of this shape
        t = {c: [] for c in CALLS}
        for rep in range(REPS):
            for c in CALLS:
                seg = segs[k]
                k += 1
                assert seg, (name, c)
                if rep >= WARM:
                    t[c].append(sum(e - s0 for s0, e, _ in seg) / 1e3)
        Ho = (H + 2 * pd - 2 * pd - 1) // s + 1
        mb = (N * H * H * C + N * Ho * Ho * C) * 2 / 1e6
        copy = t['copy fwd'] + t['copy wgrad']
        print('\n%-14s C = O = %4d, %3d x %3d -> %3d x %3d, stride %d, dilation %d, Cg %2d; activations %.0f MB; copy %.1f (%.1f - %.1f) us = %.2f TB/s'
              % (name, C, H, H, Ho, Ho, s, pd, C // GROUPS, mb, med(copy), min(copy), max(copy), mb / med(copy)))
        for what in ('fwd', 'dgrad', 'wgrad'):
            g, dn = t[what + ' grouped'], t[what + ' dense']
            good = max(g) < min(dn)
            ok = ok and good
            print('  %-5s grouped %8.1f (%.1f - %.1f)   dense %8.1f (%.1f - %.1f)   dense / grouped %5.1fx   grouped / copy %5.2fx   %s'
                  % (what, med(g), min(g), max(g), med(dn), min(dn), max(dn), med(dn) / med(g), med(g) / med(copy),
                     'faster than dense' if good else 'NOT faster than dense'))
    print('\ncondition (every grouped kernel faster than its dense counterpart, slowest grouped repetition against fastest dense): %s'
          % ('met' if ok else 'NOT met'))
    return 0 if ok else 1


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        sys.exit(report(sys.argv[2]))
    run()
