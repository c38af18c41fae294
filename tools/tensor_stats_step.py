"""The R101 SNIPER training step with the gradient guard (Trainer(skip_nonfinite=True)) and the same step with the skip report on
(Trainer(skip_nonfinite=True, skip_report=True)), alternating on one card in one process:

    python tools/tensor_stats_step.py [chips (20)] [steps per block (20)] [rounds (3)]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/tensor_stats_step.py 20 20 3
    python tools/tensor_stats_step.py --report DIR

Both train at a tiny learning rate; no step is skipped, so the report's launch pair takes its early exit on every step -- what a healthy
run pays.  Prints ms per step of every block, the C-ABI calls the report adds to an eager step, and then, ISOLATED on the reporting
trainer's gradient arena with the R101 table (nothing else running): sn_tensor_stats writing every record, its early exit, sn_grad_guard
over the same bytes (one record), and torch._foreach_norm over the per-parameter views -- host-timed with events, median of 30.

--report DIR reads the kernel trace of the same run: a step is cut at the forward max-pool launch, a reporting step is one that holds
a tensor_stats_pass_kernel launch.  IN SITU, per step, median over the steps: the early-exit launch pair; then the launches of the
isolated block (everything behind the last step), by kernel."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))

CONFIGS = (('guard', {'skip_nonfinite': True}), ('report', {'skip_nonfinite': True, 'skip_report': True}))       # label, Trainer(**options)
REPS = 30


def _timed(fn, reps=REPS):
    """median / min / max us of fn() alone on the stream (events around every call)"""
    import torch
    for _ in range(3):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    v = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
    return v[len(v) // 2], v[0], v[-1]


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
        assert (tr.mod.exe.skip_report is not None) == (label == 'report')
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
        print('%-6s %d C-ABI calls in one eager step' % (label, len(calls)), flush=True)
        trs[label] = tr
    a, b = counts['guard'], counts['report']
    print('C-ABI calls of the reporting eager step against the guarded one: ' + (', '.join(
        '%s %+d' % (n, b[n] - a[n]) for n in sorted(set(a) | set(b)) if a[n] != b[n]) or 'none'), flush=True)
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
            print('round %d %-6s %.3f ms per step (%d chips, %d steps, hipGraph replay)' % (r, label, ms[label][-1], chips, steps), flush=True)
    med = {}
    for label, _ in CONFIGS:
        v = sorted(ms[label])
        med[label] = v[len(v) // 2]
        print('%-6s median %.3f ms per step, min %.3f, max %.3f' % (label, med[label], v[0], v[-1]))
    spread = max(max(v) - min(v) for v in ms.values())
    print('the reporting step costs %+.3f ms (%+.2f %%) over the guarded one; block-to-block spread of same-kind blocks %.3f ms' % (
        med['report'] - med['guard'], 100 * (med['report'] / med['guard'] - 1), spread))
    st = trs['report'].mod.grad_guard_state()
    assert st['steps'] == 5 + rounds * steps and st['skipped'] == 0 and trs['report'].mod.skip_report() is None, st
    print('guard state after the run: %r; no step skipped, the report buffer was never written' % (st,))

    # ---- isolated: the same arena, nothing else on the card
    ex = trs['report'].mod.exe
    arena, g, tab = ex.arena_grad, ex.guard, ex.skip_report['table']
    n = arena.numel()
    lens = tab['segs'][:, 1]
    print('isolated, on the gradient arena of the reporting trainer: %d fp32 = %.1f MB in %d tensors of %d .. %d elements, %d work items' % (
        n, 4 * n / 1e6, tab['T'], lens.min(), lens.max(), tab['n_items']))
    out = torch.zeros((1 + tab['T'], 8), dtype=torch.float64, device=arena.device)
    views = [arena[o:o + k] for o, k in tab['segs'].tolist()]

    def stats(only):
        hip.call('sn_tensor_stats', arena, 1, tab['plan'], tab['n_items'], tab['T'], 0, g['state'], only, tab['ws'], out, hip.stream())

    def guard_call():
        hip.call('sn_grad_guard', arena, n, ex.hyper, g['clip_global_norm'], g['skip_nonfinite'], 0, g['ws'], g['state'], hip.stream())
    res = {}
    for what, fn in (('sn_tensor_stats, every record written', lambda: stats(0)),
                     ('sn_tensor_stats, only_if_skipped (early exit)', lambda: stats(1)),
                     ('sn_grad_guard (pass + finalize, one record)', guard_call),
                     ('torch._foreach_norm over %d views' % len(views), lambda: torch._foreach_norm(views))):
        m, lo, hi = _timed(fn)
        res[what.split(',')[0].split(' ')[0] + ('/exit' if 'early' in what else '')] = m
        print('  %-48s %8.1f us (min %.1f, max %.1f)  %.2f TB/s of %d MB' % (what, m, lo, hi, 4 * n / m / 1e6, 4 * n / 1e6), flush=True)
    print('  the full pass is %.2f x the guard\'s pass; the early exit %.1f us' % (res['sn_tensor_stats'] / res['sn_grad_guard'],
                                                                                  res['sn_tensor_stats/exit']))
    stats(0)
    norms = torch._foreach_norm(views)
    torch.cuda.synchronize()
    rec = out.cpu().numpy()
    worst = max(abs(np.sqrt(r[0]) - float(v)) / max(float(v), 1e-30) for r, v in zip(rec[1:], norms))
    print('  per-tensor norms: largest relative difference to torch (fp32 accumulation) %.3g; header %r' % (worst, rec[0].tolist()))


def report(root):
    import csv
    import glob
    from full_trunk_step import _short
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(files[0])))
    cuts = [k for k, r in enumerate(rows) if 'maxpool_kernel' in r[2]]
    segs = [rows[a:b] for a, b in zip(cuts, cuts[1:])]
    tail = rows[cuts[-1]:]
    is_on = lambda s: any('tensor_stats_pass_kernel' in r[2] for r in s)
    on, off = [s for s in segs if is_on(s)], [s for s in segs if not is_on(s)]
    assert on and off, (len(on), len(off))
    on, off = on[len(on) // 4:], off[len(off) // 4:]          # (the first quarter: eager steps, capture, warm-up)
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
    a, b = by_name(off), by_name(on)
    print('%d reporting and %d guarded steps of the trace (after the warm-up quarter of each)' % (len(on), len(off)))
    print('in situ, kernel time per step, us (median over the steps): the early-exit launch pair')
    own = 0.0
    for n in sorted(b):
        if 'tensor_stats' in n:
            own += b[n]
            print('  %-60s guarded %9.1f   reporting %9.1f' % (n[:60], a.get(n, 0.0), b[n]))
    print('  the pair %.1f us per step; sum of kernel time per step %.1f -> %.1f us (%+.1f)' % (
        own, sum(a.values()), sum(b.values()), sum(b.values()) - sum(a.values())))
    last = max([k for k, r in enumerate(tail) if 'weight_transpose_batched_kernel' in r[2]][:1] or [0])
    iso = collections.defaultdict(list)
    for r in tail[last + 1:]:
        iso[_short(r[2])].append(us(r))
    print('isolated block of the trace, per launch, us (median; launches):')
    for n, v in sorted(iso.items(), key=lambda kv: -sum(kv[1])):
        if len(v) >= REPS:
            print('  %-60s %9.1f  (%d)' % (n[:60], med(v), len(v)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        report(sys.argv[2])
    else:
        main()
