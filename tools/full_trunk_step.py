"""The R101 SNIPER training step with the config's network.FIXED_PARAMS (conv0, bn0, stage1: the stem and stage 1 frozen)
and with FIXED_PARAMS = [] (everything but bn_data trains, through the max-pool backward), alternating on one card in one process:

    python tools/full_trunk_step.py [chips (20)] [steps per block (20)] [rounds (3)]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/full_trunk_step.py 20 20 3
    python tools/full_trunk_step.py --report DIR

Both train at a tiny learning rate (the time of a step does not depend on it; bn0 and stage 1 normalise with the moving statistics
of a random initialisation).  Prints ms per step of every block, and the C-ABI calls the unfrozen eager step adds.

--report DIR reads the kernel trace of the same run: a step is cut at the forward max-pool launch (one per step either way), an
unfrozen step is one that holds a maxpool_bwd_kernel launch.  Per launch, median over the unfrozen steps: the max-pool backward;
bn0's bn_frozen_bwd_kernel (the only one that starts after the pool's: everything of stage 1 ran before it); the stem's
conv_wgrad_kernel; and the convolution launches of stage 1's backward (from the data gradient in front of the step's first
bn_frozen_bwd_kernel to the pool's backward).  The yardstick: the pool backward moves 378 MB at 20 chips (x 168, dy 42, dx 168),
bn0's backward 504 MB on the same tensor, so the pool's launch should not take longer than bn0's."""
import collections
import csv
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))

CONFIGS = (('config', None), ('[]', []))      # label, Trainer(fixed_params=...)


def main():
    chips = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    import numpy as np
    import torch
    from frozen_bn_probe import card
    from sniper_amd import hip
    from sniper_amd.train import Trainer
    print('card: ' + card(), flush=True)
    trs, counts = {}, {}
    real = hip.call
    for label, fixed in CONFIGS:
        tr = Trainer(batch_images=chips, n_images=48, seed=0, fixed_params=fixed)
        tr.mod.init_optimizer(optimizer='sgd', optimizer_params={'learning_rate': 1e-6, 'momentum': 0.9, 'wd': 1e-4})
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
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'FIXED_PARAMS=%s: step is not finite' % label
        assert tr.mod.exe._graph_fb is not None and tr.mod.exe._graph_up is not None
        n_train = sum(1 for p in tr.mod.exe.params.values() if p.trainable)
        print('FIXED_PARAMS=%-6s %d trainable parameters, %d C-ABI calls in one eager step' % (label, n_train, len(calls)), flush=True)
        trs[label] = tr
    base, full = counts['config'], counts['[]']
    print('C-ABI calls the unfrozen eager step adds: ' + ', '.join(
        '%s %+d' % (n, full[n] - base[n]) for n in sorted(set(base) | set(full)) if full[n] != base[n]), flush=True)
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
            assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'FIXED_PARAMS=%s: step is not finite' % label
            print('round %d FIXED_PARAMS=%-6s %.3f ms per step (%d chips, %d steps, hipGraph replay)' % (r, label, ms[label][-1], chips, steps),
                  flush=True)
    med = {}
    for label, _ in CONFIGS:
        v = sorted(ms[label])
        med[label] = v[len(v) // 2]
        print('FIXED_PARAMS=%-6s median %.3f ms per step, min %.3f, max %.3f' % (label, med[label], v[0], v[-1]))
    print('the unfrozen step costs %+.3f ms (%+.1f %%)' % (med['[]'] - med['config'], 100 * (med['[]'] / med['config'] - 1)))


def _short(name):
    m = re.match(r'_Z(\d+)', name)          # (a trace may hold mangled names: _Z<length><name>...)
    if m:
        return name[m.end():m.end() + int(m.group(1))]
    name = name.replace('(anonymous namespace)::', '')
    return name.split('(')[0].split('<')[0].replace('void ', '')


def report(root):
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(files[0])))
    cuts = [k for k, r in enumerate(rows) if 'maxpool_kernel' in r[2]]
    segs = [rows[a:b] for a, b in zip(cuts, cuts[1:])]
    full = [s for s in segs if any('maxpool_bwd_kernel' in r[2] for r in s)]
    froz = [s for s in segs if not any('maxpool_bwd_kernel' in r[2] for r in s)]
    assert full and froz, (len(full), len(froz))
    full, froz = full[len(full) // 4:], froz[len(froz) // 4:]          # (the first quarter: eager steps, capture, warm-up)
    med = lambda v: sorted(v)[len(v) // 2]
    us = lambda r: (r[1] - r[0]) / 1e3
    pool, bn0, stem, stage1 = [], [], [], collections.OrderedDict()
    for s in full:
        at = [k for k, r in enumerate(s) if 'maxpool_bwd_kernel' in r[2]]
        assert len(at) == 1, len(at)
        pool.append(us(s[at[0]]))
        after = [r for r in s[at[0] + 1:] if 'bn_frozen_bwd_kernel' in r[2]]
        assert len(after) == 1, len(after)           # bn0's: every other moving-statistics layer lies above the pool
        bn0.append(us(after[0]))
        wg = [r for r in s if _short(r[2]) == 'conv_wgrad_kernel']
        assert len(wg) == 1 and wg[0][0] > after[0][0], len(wg)      # the stem's: every other layer's is in the batched tables
        stem.append(us(wg[0]))
        first = min(k for k, r in enumerate(s) if 'bn_frozen_bwd_kernel' in r[2])
        lo = max(k for k in range(first) if 'conv' in s[k][2] and 'wgrad' not in s[k][2])
        per = collections.Counter()
        tot = collections.Counter()
        for r in s[lo:at[0]]:
            if 'conv' in r[2] and 'wgrad' not in r[2]:
                per[_short(r[2])] += 1
                tot[_short(r[2])] += us(r)
        for n in per:
            stage1.setdefault(n, []).append((per[n], tot[n]))
    print('%d unfrozen and %d frozen steps of the trace (after the warm-up quarter of each)' % (len(full), len(froz)))
    print('maxpool_bwd_kernel                 %8.1f us per launch (min %.1f, max %.1f): 378 MB -> %.2f TB/s' % (
        med(pool), min(pool), max(pool), 378e6 / med(pool) / 1e6))
    print("bn0's bn_frozen_bwd_kernel         %8.1f us per launch (min %.1f, max %.1f): 504 MB -> %.2f TB/s" % (
        med(bn0), min(bn0), max(bn0), 504e6 / med(bn0) / 1e6))
    print('ratio pool backward / bn0 backward %8.2f  (the yardstick: <= 1)' % (med(pool) / med(bn0)))
    print("the stem's conv_wgrad_kernel       %8.1f us per step (min %.1f, max %.1f)" % (med(stem), min(stem), max(stem)))
    print("stage 1's backward, convolution data-gradient launches (main stream, between stage 2 and the pool):")
    for n, v in stage1.items():
        print('  %-40s %2d launches, %8.1f us per launch, %8.1f us per step' % (
            n, med([c for c, _ in v]), med([t / c for c, t in v]), med([t for _, t in v])))

    def by_name(group):
        per = []
        for s in group:
            c = collections.Counter()
            for r in s:
                c[_short(r[2])] += us(r)
            per.append(c)
        return {n: med([c.get(n, 0.0) for c in per]) for n in set().union(*per)}
    a, b = by_name(froz), by_name(full)
    print('kernel time per step by kernel, us (frozen -> unfrozen), where it differs by more than 20 us:')
    for n in sorted(set(a) | set(b), key=lambda n: -(b.get(n, 0) - a.get(n, 0))):
        d = b.get(n, 0) - a.get(n, 0)
        if abs(d) > 20:
            print('  %-40s %9.1f -> %9.1f  (%+.1f)' % (n, a.get(n, 0), b.get(n, 0), d))
    print('sum of kernel time per step: %.1f -> %.1f us' % (sum(a.values()), sum(b.values())))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        report(sys.argv[2])
    else:
        main()
