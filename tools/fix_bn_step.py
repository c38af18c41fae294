"""The R101 SNIPER training step with and without fix_bn, alternating on one card in one process (the whole-step A/B of
tools/ab.sh for a constructor argument instead of an environment switch):

    python tools/fix_bn_step.py [chips (20)] [steps per block (20)] [rounds (3)]

fix_bn=False is the step bench.py measures (forward + backward + SGD on one resident batch; without bench.py's anchor labelling);
fix_bn=True normalises every BatchNorm of stages 2 - 4 with moving statistics.  Both train at a tiny learning rate (the time of a
step does not depend on it, and a randomly initialised fix_bn network does not survive the config's).  Prints ms per step of every
block and the C-ABI calls one eager step issues."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'probes'))


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
    for fix_bn in (False, True):
        tr = Trainer(batch_images=chips, n_images=48, seed=0, fix_bn=fix_bn)
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
        counts[fix_bn] = calls
        for _ in range(4):                   # second eager step, capture, replays
            outs = tr.step(tr.batch)
        torch.cuda.synchronize()
        assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'fix_bn=%s: step is not finite' % fix_bn
        assert tr.mod.exe._graph_fb is not None and tr.mod.exe._graph_up is not None
        trs[fix_bn] = tr
    for fix_bn in (False, True):
        c = counts[fix_bn]
        bn = sorted(set(n for n in c if n.startswith('sn_bn_') or n in ('sn_conv_fwd_stats', 'sn_conv_dgrad_bn')))
        print('fix_bn=%-5s C-ABI calls of one eager step: %d; BatchNorm family: %s' % (
            fix_bn, len(c), ', '.join('%s %d' % (n, c.count(n)) for n in bn)), flush=True)
    ms = {False: [], True: []}
    for r in range(rounds):
        for fix_bn in (False, True):
            tr = trs[fix_bn]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                outs = tr.step(tr.batch)
            torch.cuda.synchronize()
            ms[fix_bn].append((time.perf_counter() - t0) / steps * 1e3)
            assert all(np.isfinite(o.asnumpy()).all() for o in outs), 'fix_bn=%s: step is not finite' % fix_bn
            print('round %d fix_bn=%-5s %.3f ms per step (%d chips, %d steps, hipGraph replay)' % (r, fix_bn, ms[fix_bn][-1], chips, steps),
                  flush=True)
    for fix_bn in (False, True):
        v = sorted(ms[fix_bn])
        print('fix_bn=%-5s median %.3f ms per step, min %.3f, max %.3f' % (fix_bn, v[len(v) // 2], v[0], v[-1]))


if __name__ == '__main__':
    main()
