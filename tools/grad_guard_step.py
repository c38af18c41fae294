"""The R101 SNIPER training step without and with the gradient guard (Trainer(skip_nonfinite=True, clip_global_norm=...)),
alternating on one card in one process:

    python tools/grad_guard_step.py [chips (20)] [steps per block (20)] [rounds (3)]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/grad_guard_step.py 20 20 3
    python tools/grad_guard_step.py --report DIR

Both train at a tiny learning rate (the time of a step does not depend on it); the threshold is far above the norm, so the guarded
update takes its plain statement -- what a healthy run pays.  Prints ms per step of every block, the C-ABI calls the guarded eager
step issues instead of the plain update's, and then, ISOLATED on the guarded trainer's gradient arena (nothing else running, the
arena as the last step left it): the guard's two launches, the torch two-pass equivalent (torch.linalg.vector_norm +
torch.isfinite(...).all()), the plain and the guarded update of every group -- host-timed with events, median of 30.

--report DIR reads the kernel trace of the same run: a step is cut at the forward max-pool launch (one per step either way), a
guarded step is one that holds a grad_guard_partial_kernel launch.  IN SITU, per step, median over the steps: the guard's two kernels
and the guarded update kernels beside the plain update kernels; then the launches of the isolated block (everything behind the last
step), by kernel."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))

CONFIGS = (('off', {}), ('on', {'skip_nonfinite': True, 'clip_global_norm': 1e12}))       # label, Trainer(**guard options)
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
    for label, guard in CONFIGS:
        tr = Trainer(batch_images=chips, n_images=48, seed=0, **guard)
        tr.mod.init_optimizer(optimizer='sgd', optimizer_params=dict(optimizer_params(tr.cfg), learning_rate=1e-6, momentum=0.9, wd=1e-4))
        assert (tr.mod.exe.guard is not None) == bool(guard)
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
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'guard %s: step is not finite' % label
        assert tr.mod.exe._graph_fb is not None and tr.mod.exe._graph_up is not None, 'guard %s: the step is not replayed' % label
        print('guard %-3s %d C-ABI calls in one eager step; state %r' % (label, len(calls), tr.mod.grad_guard_state()), flush=True)
        trs[label] = tr
    off, on = counts['off'], counts['on']
    print('C-ABI calls of the guarded eager step against the plain one: ' + ', '.join(
        '%s %+d' % (n, on[n] - off[n]) for n in sorted(set(off) | set(on)) if on[n] != off[n]), flush=True)
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
            assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'guard %s: step is not finite' % label
            print('round %d guard %-3s %.3f ms per step (%d chips, %d steps, hipGraph replay)' % (r, label, ms[label][-1], chips, steps), flush=True)
    med = {}
    for label, _ in CONFIGS:
        v = sorted(ms[label])
        med[label] = v[len(v) // 2]
        print('guard %-3s median %.3f ms per step, min %.3f, max %.3f' % (label, med[label], v[0], v[-1]))
    spread = max(max(v) - min(v) for v in ms.values())
    print('the guarded step costs %+.3f ms (%+.2f %%); run-to-run spread of a block %.3f ms' % (
        med['on'] - med['off'], 100 * (med['on'] / med['off'] - 1), spread))
    st = trs['on'].mod.grad_guard_state()
    assert st['steps'] == 5 + rounds * steps and st['skipped'] == 0, st
    print('guard state after the run: %r' % (st,))

    # ---- isolated: the same arena, nothing else on the card
    ex, plain = trs['on'].mod.exe, trs['off'].mod.exe
    arena, g = ex.arena_grad, ex.guard
    n = arena.numel()
    print('isolated, on the gradient arena of the guarded trainer: %d fp32 = %.1f MB (the last-level cache holds 256 MiB)' % (n, 4 * n / 1e6))

    def guard_call():
        hip.call('sn_grad_guard', arena, n, ex.hyper, g['clip_global_norm'], g['skip_nonfinite'], 0, g['ws'], g['state'], hip.stream())

    def torch_two_pass():
        return torch.linalg.vector_norm(arena), torch.isfinite(arena).all()

    def update(e, guarded):
        for (lr_mult, wd_mult, _half), a, b in e.groups:
            if guarded:
                hip.call('sn_sgd_mom_update_guarded_dev', e.arena_master[a:], e.arena_grad[a:], e.arena_mom[a:], e.arena_w16[a:], b - a,
                         e.hyper, float(lr_mult), float(wd_mult), g['clip_gradient'], g['state'], hip.stream())
            else:
                hip.call('sn_sgd_mom_update_dev', e.arena_master[a:], e.arena_grad[a:], e.arena_mom[a:], e.arena_w16[a:], b - a,
                         e.hyper, float(lr_mult), float(wd_mult), hip.stream())
    for what, fn, nbytes in (('sn_grad_guard (pass + finalize)', guard_call, 4 * n),
                             ('torch vector_norm + isfinite().all()', torch_two_pass, 8 * n),
                             ('sn_sgd_mom_update_dev, %d groups' % len(plain.groups), lambda: update(plain, False), 22 * n),
                             ('sn_sgd_mom_update_guarded_dev, %d groups' % len(ex.groups), lambda: update(ex, True), 22 * n)):
        m, lo, hi = _timed(fn)
        print('  %-44s %8.1f us (min %.1f, max %.1f)  %.2f TB/s of %d MB' % (what, m, lo, hi, nbytes / m / 1e6, nbytes / 1e6), flush=True)
    nrm, fin = torch_two_pass()
    guard_call()
    torch.cuda.synchronize()
    dev_norm = float(g['state'][0])
    print('  norm: guard %.9g, torch (fp32 accumulation) %.9g, all finite %s' % (dev_norm, float(nrm), bool(fin)))


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
    is_on = lambda s: any('grad_guard_partial_kernel' in r[2] for r in s)
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
    print('%d guarded and %d plain steps of the trace (after the warm-up quarter of each)' % (len(on), len(off)))
    print('in situ, kernel time per step, us (median over the steps):')
    for n in ('grad_guard_partial_kernel', 'grad_guard_finalize_kernel', 'sgd_guard_vec4_kernel', 'sgd_guard_kernel',
              'sgd_dev_vec4_kernel', 'sgd_dev_kernel'):
        print('  %-40s plain %9.1f   guarded %9.1f' % (n, a.get(n, 0.0), b.get(n, 0.0)))
    own = sum(b.get(n, 0.0) for n in ('grad_guard_partial_kernel', 'grad_guard_finalize_kernel'))
    upd = sum(b.get(n, 0.0) for n in ('sgd_guard_vec4_kernel', 'sgd_guard_kernel')) - sum(a.get(n, 0.0) for n in ('sgd_dev_vec4_kernel', 'sgd_dev_kernel'))
    print('  the guard itself %.1f us per step; guarded update against plain update %+.1f us' % (own, upd))
    print('kernel time per step by kernel, us (plain -> guarded), where it differs by more than 5 us:')
    for n in sorted(set(a) | set(b), key=lambda n: -(b.get(n, 0) - a.get(n, 0))):
        d = b.get(n, 0) - a.get(n, 0)
        if abs(d) > 5:
            print('  %-40s %9.1f -> %9.1f  (%+.1f)' % (n, a.get(n, 0), b.get(n, 0), d))
    print('sum of kernel time per step: %.1f -> %.1f us (%+.1f)' % (sum(a.values()), sum(b.values()), sum(b.values()) - sum(a.values())))
    # the isolated block: behind the last step's optimizer pass (its last weight_transpose / bn scale-shift launch)
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
