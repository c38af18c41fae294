"""The R101 SNIPER training step with one update per batch (k = 1) and with gradient accumulation (Trainer(accumulate=k): one update
per k batches on the sum of their gradients), alternating on one card in one process:

    python tools/accumulate_step.py [chips (20)] [k (4)] [windows per block (5)] [rounds (3)]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/accumulate_step.py 20 4 5 3
    python tools/accumulate_step.py --report DIR [floats in the arena]

Both train at a tiny learning rate (the time of a step does not depend on it).  A block is `windows` x k micro-batches either way;
prints ms per MICRO-BATCH of every block, and the C-ABI calls a micro-step and a window's end issue against the k = 1 step (counted
over one eager window).  The yardstick of the step is the k = 1 block of the same process; the margin is the spread between blocks of
the same kind.  The expectation -- nobody has measured it before this tool -- is one stream pass per micro-step (8 bytes per trainable
parameter for the copy, 12 for the add) against k - 1 saved optimizer passes per window.

The program ends with the yardstick of the kernel: YARD rounds of [sn_grad_accumulate copy, sn_grad_accumulate add, torch's
acc.copy_(grad), torch's acc.add_(grad)] on the accumulating executor's own two arenas, and nothing after them.  --report DIR reads
the kernel trace of the same run: the last 4 x YARD launches are that yardstick (checked: two grad_accum_kernel launches, then one
launch each of torch's); the grad_accum_kernel launches before them are the ones of the steps, in situ.  With the arena's size in
floats (printed by the run) the times become bytes per second."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))

YARD = 20


def _counted(hip, fn):
    real, calls = hip.call, []

    def counting(name, *args):
        calls.append(name)
        return real(name, *args)
    hip.call = counting
    try:
        fn()
    finally:
        hip.call = real
    return collections.Counter(calls)


def _diff(a, b):
    return ', '.join('%s %+d' % (n, b[n] - a[n]) for n in sorted(set(a) | set(b)) if a[n] != b[n]) or 'none'


def main():
    chips = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    k = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    windows = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    assert k > 1, 'k must be > 1 (the k = 1 step is the yardstick)'
    import numpy as np
    import torch
    from frozen_bn_probe import card
    from sniper_amd import hip
    from sniper_amd.train import Trainer, optimizer_params
    print('card: ' + card(), flush=True)
    configs = (('k=1', 1), ('k=%d' % k, k))
    trs, counts = {}, {}
    for label, kk in configs:
        tr = Trainer(batch_images=chips, n_images=48, seed=0, accumulate=kk)
        tr.mod.init_optimizer(optimizer='sgd', optimizer_params=dict(optimizer_params(tr.cfg), learning_rate=1e-6, momentum=0.9, wd=1e-4))
        ex = tr.mod.exe
        assert (ex.accum is not None) == (kk > 1) and tr.mod.accumulate_state()['k'] == kk
        graphs, ex.use_graphs = ex.use_graphs, False          # one eager window: every launch goes through hip.call
        counts[label] = [_counted(hip, lambda: tr.step(tr.batch)) for _ in range(kk)]
        ex.use_graphs = graphs
        for _ in range(4 * kk):                               # a second eager update, the captures, replays
            outs = tr.step(tr.batch)
        torch.cuda.synchronize()
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), '%s: step is not finite' % label
        assert ex._graph_fb is not None and ex._graph_up is not None, '%s: the step is not replayed' % label
        assert tr.mod.accumulate_state() == {'k': kk, 'pending': 0, 'updates': 5}, tr.mod.accumulate_state()
        print('%-5s %s C-ABI calls in the eager steps of one window; arena %d floats' % (
            label, ' + '.join(str(sum(c.values())) for c in counts[label]), ex.arena_grad.numel()), flush=True)
        trs[label] = tr
    plain, acc = counts['k=1'][0], counts['k=%d' % k]
    print('C-ABI calls of the first micro-step of a window against the k = 1 step: ' + _diff(plain, acc[0]), flush=True)
    print('C-ABI calls of a later micro-step against the first: ' + _diff(acc[0], acc[1]) if k > 2 else '(k = 2: no middle micro-step)', flush=True)
    print('C-ABI calls of the window\'s last micro-step against the k = 1 step: ' + _diff(plain, acc[-1]), flush=True)
    ms = {label: [] for label, _ in configs}
    steps = windows * k
    for r in range(rounds):
        for label, kk in configs:
            tr = trs[label]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                outs = tr.step(tr.batch)
            torch.cuda.synchronize()
            ms[label].append((time.perf_counter() - t0) / steps * 1e3)
            assert all(np.isfinite(o.asnumpy()).all() for o in outs), '%s: step is not finite' % label
            print('round %d %-5s %.3f ms per micro-batch (%d chips, %d micro-batches, %d updates, hipGraph replay)' % (
                r, label, ms[label][-1], chips, steps, steps // kk), flush=True)
    med = {}
    for label, _ in configs:
        v = sorted(ms[label])
        med[label] = v[len(v) // 2]
        print('%-5s median %.3f ms per micro-batch, min %.3f, max %.3f' % (label, med[label], v[0], v[-1]))
    spread = max(max(v) - min(v) for v in ms.values())
    a, b = med['k=1'], med['k=%d' % k]
    print('a micro-batch of the accumulating step costs %+.3f ms (%+.2f %%) over the k = 1 step; spread between blocks of a kind %.3f ms' % (
        b - a, 100 * (b / a - 1), spread))
    for label, kk in configs:
        st = trs[label].mod.accumulate_state()
        assert st == {'k': kk, 'pending': 0, 'updates': 5 + rounds * steps // kk}, (label, st)
        print('%-5s accumulate_state after the run: %r, num_update %d' % (label, st, trs[label].mod.exe.num_update))
    # the kernel's yardstick, last in the program (--report reads it by position)
    ex = trs['k=%d' % k].mod.exe
    arena, grad, n = ex.accum['arena'], ex.arena_grad, ex.arena_grad.numel()
    grad.normal_()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(YARD)]
    for r in range(YARD):
        ev[r][0].record()
        hip.call('sn_grad_accumulate', arena, grad, n, 1, 0, hip.stream())
        ev[r][1].record()
        hip.call('sn_grad_accumulate', arena, grad, n, 0, 0, hip.stream())
        ev[r][2].record()
        arena.copy_(grad)
        ev[r][3].record()
        arena.add_(grad)
        ev[r][4].record()
    torch.cuda.synchronize()
    names = ('sn_grad_accumulate copy', 'sn_grad_accumulate add', 'torch acc.copy_(grad)', 'torch acc.add_(grad)')
    for j, (what, nbytes) in enumerate(zip(names, (8, 12, 8, 12))):
        t = sorted(ev[r][j].elapsed_time(ev[r][j + 1]) for r in range(YARD // 4, YARD))
        m = t[len(t) // 2]
        print('%-24s %8.1f us between events (median of %d, min %.1f, max %.1f): %d bytes per float, %.2f TB/s' % (
            what, m * 1e3, len(t), t[0] * 1e3, t[-1] * 1e3, nbytes, nbytes * n / (m * 1e-3) / 1e12))
    print('arena: %d floats (%.1f MB each); event times include the launch gap, the kernel trace (--report) does not' % (n, 4e-6 * n))


def report(root, n=None):
    import csv
    import glob
    from full_trunk_step import _short
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(files[0])))
    med = lambda v: sorted(v)[len(v) // 2]
    us = lambda r: (r[1] - r[0]) / 1e3
    is_copy = lambda name: 'ILb1E' in name.split('grad_accum_kernel')[1][:8] or 'grad_accum_kernel<true' in name
    yard, rest = rows[-4 * YARD:], rows[:-4 * YARD]
    assert len(yard) == 4 * YARD, len(rows)
    cols = [yard[j::4] for j in range(4)]
    assert all('grad_accum_kernel' in r[2] for r in cols[0] + cols[1]), sorted(set(r[2] for r in cols[0] + cols[1]))
    assert all(is_copy(r[2]) for r in cols[0]) and not any(is_copy(r[2]) for r in cols[1])
    for c in cols[2:]:
        assert len(set(r[2] for r in c)) == 1 and 'grad_accum_kernel' not in c[0][2], sorted(set(r[2] for r in c))
    rate = lambda t, nbytes: '' if n is None else ', %.2f TB/s' % (nbytes * n / (t * 1e-6) / 1e12)
    print('the yardstick (the last %d launches of the trace, after a warm-up quarter), kernel time, us, median:' % (4 * YARD))
    for c, what, nbytes in zip(cols, ('sn_grad_accumulate copy', 'sn_grad_accumulate add', 'torch acc.copy_(grad)', 'torch acc.add_(grad)'),
                               (8, 12, 8, 12)):
        t = [us(r) for r in c[YARD // 4:]]
        print('  %-24s %8.1f (min %.1f, max %.1f)%s   %s' % (what, med(t), min(t), max(t), rate(med(t), nbytes), _short(c[0][2])))
    situ = [r for r in rest if 'grad_accum_kernel' in r[2]]
    assert situ, 'no accumulate launch in the steps of the trace'
    situ = situ[len(situ) // 4:]                              # (the first quarter: eager steps, capture, warm-up)
    for what, sel, nbytes in (('copy', True, 8), ('add', False, 12)):
        t = [us(r) for r in situ if is_copy(r[2]) == sel]
        print('in situ (beside the replayed graph), %-4s: %8.1f us median of %d launches (min %.1f, max %.1f)%s' % (
            what, med(t), len(t), min(t), max(t), rate(med(t), nbytes)))
    # what a window saves: the optimizer pass (update kernels + the refresh of the compute copies) runs once per k micro-batches
    cuts = [i for i, r in enumerate(rest) if 'maxpool_kernel' in r[2]]
    segs = [rest[a:b] for a, b in zip(cuts, cuts[1:])]
    segs = segs[len(segs) // 4:]
    has = lambda s, frag: any(frag in r[2] for r in s)
    groups = {'k = 1 step': [s for s in segs if has(s, 'sgd_dev') and not has(s, 'grad_accum_kernel')],
              'micro-step without update': [s for s in segs if not has(s, 'sgd_dev') and has(s, 'grad_accum_kernel')],
              'window\'s last micro-step': [s for s in segs if has(s, 'sgd_dev') and has(s, 'grad_accum_kernel')]}
    print('kernel time per micro-batch, us (median over the segments between two forward max-pool launches):')
    for what, g in groups.items():
        if g:
            print('  %-28s %10.1f   (%d segments)' % (what, med([sum(us(r) for r in s) for s in g]), len(g)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        report(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else None)
    else:
        main()
