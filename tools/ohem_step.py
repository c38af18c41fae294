"""The R101 SNIPER training step without and with online hard example mining (TRAIN.ENABLE_OHEM: Trainer(ohem=256)), alternating
on one card in one process:

    python tools/ohem_step.py [chips (20)] [steps per block (20)] [rounds (3)]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/ohem_step.py 20 20 3
    python tools/ohem_step.py --report DIR

Both train at a tiny learning rate (the time of a step does not depend on it).  Prints ms per step of every block and the C-ABI
calls the OHEM eager step adds (one sn_box_annotator_ohem; its seven reshapes are views, not calls).

--report DIR reads the kernel trace of the same run: a step is cut at the forward max-pool launch (one per step either way), an
OHEM step is one that holds a box_annotator_ohem_kernel launch.  Per launch, median over the OHEM steps: the operator, and the
softmax_fwd_kernel of the cls_prob node -- the first one after the operator, on the same (B * R, C) scores.  That is the existing
kernel that reads the same bytes, so it is the yardstick: the operator does the softmax's work plus a box loss plus a ranking of
R keys per image, and the bar is 3 x the softmax launch (an allowance for the ranking, not a measured ratio)."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))

OHEM_ROIS = 256                                    # BATCH_ROIS_OHEM of every shipped yml
CONFIGS = (('off', None), ('on', OHEM_ROIS))       # label, Trainer(ohem=...)


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
    for label, ohem in CONFIGS:
        tr = Trainer(batch_images=chips, n_images=48, seed=0, ohem=ohem)
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
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'ENABLE_OHEM %s: step is not finite' % label
        assert tr.mod.exe._graph_fb is not None and tr.mod.exe._graph_up is not None, 'ENABLE_OHEM %s: the step is not replayed' % label
        kept = (outs[4].asnumpy().reshape(chips, -1) >= 0).sum(1)
        print('ENABLE_OHEM %-3s %d C-ABI calls in one eager step; labelled RoIs per chip that reach the losses: min %d, max %d' % (
            label, len(calls), kept.min(), kept.max()), flush=True)
        trs[label] = tr
    off, on = counts['off'], counts['on']
    print('C-ABI calls the OHEM eager step adds: ' + ', '.join(
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
            assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'ENABLE_OHEM %s: step is not finite' % label
            print('round %d ENABLE_OHEM %-3s %.3f ms per step (%d chips, %d steps, hipGraph replay)' % (r, label, ms[label][-1], chips, steps),
                  flush=True)
    med = {}
    for label, _ in CONFIGS:
        v = sorted(ms[label])
        med[label] = v[len(v) // 2]
        print('ENABLE_OHEM %-3s median %.3f ms per step, min %.3f, max %.3f' % (label, med[label], v[0], v[-1]))
    print('the OHEM step costs %+.3f ms (%+.2f %%)' % (med['on'] - med['off'], 100 * (med['on'] / med['off'] - 1)))


def report(root):
    import csv
    import glob
    from full_trunk_step import _short
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = sorted((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in csv.DictReader(open(files[0])))
    cuts = [k for k, r in enumerate(rows) if 'maxpool_kernel' in r[2]]
    segs = [rows[a:b] for a, b in zip(cuts, cuts[1:])]
    on = [s for s in segs if any('box_annotator_ohem_kernel' in r[2] for r in s)]
    off = [s for s in segs if not any('box_annotator_ohem_kernel' in r[2] for r in s)]
    assert on and off, (len(on), len(off))
    on, off = on[len(on) // 4:], off[len(off) // 4:]          # (the first quarter: eager steps, capture, warm-up)
    med = lambda v: sorted(v)[len(v) // 2]
    us = lambda r: (r[1] - r[0]) / 1e3
    ohem, soft = [], []
    for s in on:
        at = [k for k, r in enumerate(s) if 'box_annotator_ohem_kernel' in r[2]]
        assert len(at) == 1, len(at)                  # one launch per step
        ohem.append(us(s[at[0]]))
        after = [r for r in s[at[0] + 1:] if 'softmax_fwd_kernel' in r[2]]
        assert after, 'no softmax_fwd_kernel after the operator'
        soft.append(us(after[0]))
    print('%d OHEM and %d plain steps of the trace (after the warm-up quarter of each)' % (len(on), len(off)))
    print('box_annotator_ohem_kernel          %8.1f us per launch (min %.1f, max %.1f), one launch per step' % (med(ohem), min(ohem), max(ohem)))
    print("cls_prob's softmax_fwd_kernel      %8.1f us per launch (min %.1f, max %.1f), the same scores" % (med(soft), min(soft), max(soft)))
    print('ratio operator / softmax           %8.2f  (the bar: <= 3)' % (med(ohem) / med(soft)))

    def by_name(group):
        per = []
        for s in group:
            c = collections.Counter()
            for r in s:
                c[_short(r[2])] += us(r)
            per.append(c)
        return {n: med([c.get(n, 0.0) for c in per]) for n in set().union(*per)}
    a, b = by_name(off), by_name(on)
    print('kernel time per step by kernel, us (plain -> OHEM), where it differs by more than 5 us:')
    for n in sorted(set(a) | set(b), key=lambda n: -(b.get(n, 0) - a.get(n, 0))):
        d = b.get(n, 0) - a.get(n, 0)
        if abs(d) > 5:
            print('  %-40s %9.1f -> %9.1f  (%+.1f)' % (n, a.get(n, 0), b.get(n, 0), d))
    print('sum of kernel time per step: %.1f -> %.1f us' % (sum(a.values()), sum(b.values())))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        report(sys.argv[2])
    else:
        main()
