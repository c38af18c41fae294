"""The R101 SNIPER training step with the static loss scale behind the gradient guard (Trainer(skip_nonfinite=True)) and with dynamic
loss scaling (Trainer(dynamic_loss_scale=True)), alternating on one card in one process:

    python tools/loss_scale_step.py [chips (20)] [steps per block (20)] [rounds (3)]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/loss_scale_step.py 20 20 3
    python tools/loss_scale_step.py --report DIR

Both train at a tiny learning rate (the time of a step does not depend on it) and neither skips a step: what a healthy run pays for
keeping the scale on the device.  Prints ms per step of every block and the C-ABI calls the scaled eager step issues instead of the
guarded static one's.  The yardstick is the guarded static step of the same process; the margin is the spread between blocks of the
same kind.

--report DIR reads the kernel trace of the same run: a step is cut at the forward max-pool launch (one per step either way), a
dynamic step is one that holds a grad_guard_scaled_finalize_kernel launch.  Per step, median over the steps: the restore and the save
launch of sn_aux_shadow (inside such a segment the first is this step's restore, the second the next step's save),
sn_grad_guard_scaled's two kernels beside sn_grad_guard's, the scaled loss kernels beside the plain ones, and every kernel whose time
per step differs by more than 5 us."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))

CONFIGS = (('static', {'skip_nonfinite': True}), ('dynamic', {'dynamic_loss_scale': True}))       # label, Trainer(**options)


def main():
    chips = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    import numpy as np
    import torch
    from frozen_bn_probe import card
    from sniper_amd import hip
    from sniper_amd.train import Trainer, optimizer_params
    print('card: ' + card(), flush=True)
    trs, counts = {}, {}
    real = hip.call
    for label, opts in CONFIGS:
        tr = Trainer(batch_images=chips, n_images=48, seed=0, **opts)
        tr.mod.init_optimizer(optimizer='sgd', optimizer_params=dict(optimizer_params(tr.cfg), learning_rate=1e-6, momentum=0.9, wd=1e-4))
        assert tr.mod.exe.guard is not None and (tr.mod.exe.loss_scale is not None) == (label == 'dynamic')
        calls = []

        def counting(name, *args):
            calls.append(name)
            return real(name, *args)
        hip.call = counting                  # the first step is eager: every launch goes through hip.call
        try:
            tr.step(tr.batch)
        finally:
            hip.call = real
        counts[label] = collections.Counter(calls)
        for _ in range(4):                   # second eager step, capture, replays
            outs = tr.step(tr.batch)
        torch.cuda.synchronize()
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), '%s: step is not finite' % label
        assert tr.mod.exe._graph_fb is not None and tr.mod.exe._graph_up is not None, '%s: the step is not replayed' % label
        print('%-7s %d C-ABI calls in one eager step; guard %r; scaler %r' % (
            label, len(calls), tr.mod.grad_guard_state(), tr.mod.loss_scale_state()), flush=True)
        trs[label] = tr
    a, b = counts['static'], counts['dynamic']
    print('C-ABI calls of the scaled eager step against the guarded static one: ' + ', '.join(
        '%s %+d' % (n, b[n] - a[n]) for n in sorted(set(a) | set(b)) if a[n] != b[n]), flush=True)
    ls = trs['dynamic'].mod.exe.loss_scale
    print('sn_aux_shadow table: %d vectors, %d floats' % (ls['n_aux'], sum(t.numel() for t in ls['aux'])), flush=True)
    ms = {label: [] for label, _ in CONFIGS}
    for r in range(rounds):
        for label, _ in CONFIGS:
            tr = trs[label]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                outs = tr.step(tr.batch)
            torch.cuda.synchronize()
            ms[label].append((time.perf_counter() - t0) / steps * 1e3)
            assert all(np.isfinite(o.asnumpy()).all() for o in outs), '%s: step is not finite' % label
            print('round %d %-7s %.3f ms per step (%d chips, %d steps, hipGraph replay)' % (r, label, ms[label][-1], chips, steps), flush=True)
    med = {}
    for label, _ in CONFIGS:
        v = sorted(ms[label])
        med[label] = v[len(v) // 2]
        print('%-7s median %.3f ms per step, min %.3f, max %.3f' % (label, med[label], v[0], v[-1]))
    spread = max(max(v) - min(v) for v in ms.values())
    print('the dynamically scaled step costs %+.3f ms (%+.2f %%) over the guarded static one; spread between blocks of a kind %.3f ms' % (
        med['dynamic'] - med['static'], 100 * (med['dynamic'] / med['static'] - 1), spread))
    for label, _ in CONFIGS:
        st = trs[label].mod.grad_guard_state()
        assert st['steps'] == 5 + rounds * steps and st['skipped'] == 0, (label, st)
        print('%-7s guard state after the run: %r' % (label, st))
    st = trs['dynamic'].mod.loss_scale_state()
    assert st['backoffs'] == 0 and st['clean'] == 5 + rounds * steps, st
    print('scaler state after the run: %r' % (st,))


def report(root):
    import csv
    import glob
    from full_trunk_step import _short
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(files[0])))
    cuts = [k for k, r in enumerate(rows) if 'maxpool_kernel' in r[2]]
    segs = [rows[a:b] for a, b in zip(cuts, cuts[1:])]
    is_dyn = lambda s: any('grad_guard_scaled_finalize_kernel' in r[2] for r in s)
    dyn, sta = [s for s in segs if is_dyn(s)], [s for s in segs if not is_dyn(s)]
    assert dyn and sta, (len(dyn), len(sta))
    dyn, sta = dyn[len(dyn) // 4:], sta[len(sta) // 4:]          # (the first quarter: eager steps, capture, warm-up)
    # a static segment right before a dynamic block holds that block's first save launch: leave such segments out
    sta = [s for s in sta if not any('aux_shadow_kernel' in r[2] for r in s)]
    med = lambda v: sorted(v)[len(v) // 2]
    us = lambda r: (r[1] - r[0]) / 1e3

    def by_name(group):
        per = []
        for s in group:
            c = collections.Counter()
            for r in s:
                c[_short(r[2])] += us(r)
            per.append(c)
        return {n: med([c.get(n, 0.0) for c in per]) for n in set().union(*per)}
    a, b = by_name(sta), by_name(dyn)
    print('%d dynamic and %d static guarded steps of the trace (after the warm-up quarter of each)' % (len(dyn), len(sta)))
    shadow = [[us(r) for r in s if 'aux_shadow_kernel' in r[2]] for s in dyn]
    both = [v for v in shadow if len(v) == 2]
    if both:
        print('sn_aux_shadow, per launch, us (median over %d steps): restore (nothing skipped: reads the flag, writes nothing) %.1f, '
              'save %.1f' % (len(both), med([v[0] for v in both]), med([v[1] for v in both])))
    print('in situ, kernel time per step, us (median over the steps):')
    names = ('aux_shadow_kernel', 'grad_guard_partial_kernel', 'grad_guard_finalize_kernel', 'grad_guard_scaled_finalize_kernel',
             'softmax_bwd_kernel', 'softmax_bwd_scaled_kernel', 'softmax_rows_bwd_kernel', 'softmax_rows_bwd_scaled_kernel',
             'ew_f32_kernel', 'fill_scaled_kernel', 'sgd_guard_vec4_kernel', 'sgd_guard_kernel')
    for n in names:
        print('  %-40s static %9.1f   dynamic %9.1f' % (n, a.get(n, 0.0), b.get(n, 0.0)))
    new = b.get('aux_shadow_kernel', 0.0)
    print('  the two new launches %.1f us per step; guard %+.1f us; loss-gradient kernels %+.1f us; guarded update %+.1f us' % (
        new, sum(b.get(n, 0.0) - a.get(n, 0.0) for n in names[1:4]), sum(b.get(n, 0.0) - a.get(n, 0.0) for n in names[4:10]),
        sum(b.get(n, 0.0) - a.get(n, 0.0) for n in names[10:])))
    print('kernel time per step by kernel, us (static -> dynamic), where it differs by more than 5 us:')
    for n in sorted(set(a) | set(b), key=lambda n: -(b.get(n, 0) - a.get(n, 0))):
        d = b.get(n, 0) - a.get(n, 0)
        if abs(d) > 5:
            print('  %-40s %9.1f -> %9.1f  (%+.1f)' % (n, a.get(n, 0), b.get(n, 0), d))
    print('sum of kernel time per step: %.1f -> %.1f us (%+.1f)' % (sum(a.values()), sum(b.values()), sum(b.values()) - sum(a.values())))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        report(sys.argv[2])
    else:
        main()
