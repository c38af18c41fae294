"""sn_bn_backward (batch statistics: reduce + finalize + dx) against sn_bn_frozen_backward (moving statistics, fix_bn) on the six
BatchNorm launch shapes of the C2 step, ReLU and `accumulate`, alternating in one process:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o k -- python tools/probes/frozen_bn_probe.py
    python tools/probes/frozen_bn_probe.py --report DIR          # per shape: kernel time of every variant, from the trace

One repetition launches, in this order: the batch-statistics backward (baseline), the frozen backward (dx + parameter gradients in
one pass), its dx-only call followed by its parameter-only call (the "wide dx + reduce" pair), and the baseline again (the spread of
the baseline within the run).  The report sums the kernels of each call from their start / end timestamps."""
import csv
import glob
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SHAPES = [(81920, 128), (81920, 512), (20480, 256), (20480, 1024), (20480, 512), (20480, 2048)]
REPS, WARM = 23, 3
# kernels of one repetition, in launch order: (variant, kernel name fragment)
SEQ = [('baseline', 'bn_bwd_reduce_kernel'), ('baseline', 'bn_bwd_finalize_kernel'), ('baseline', 'bn_bwd_dx_kernel'),
       ('frozen', ('bn_frozen_bwd_kernelILb1ELb1', 'bn_frozen_bwd_kernel<true, true>')), ('frozen', 'bn_frozen_finalize_kernel'),
       ('dx_only', ('bn_frozen_bwd_kernelILb1ELb0', 'bn_frozen_bwd_kernel<true, false>')),
       ('par_only', ('bn_frozen_bwd_kernelILb0ELb1', 'bn_frozen_bwd_kernel<false, true>')), ('par_only', 'bn_frozen_finalize_kernel'),
       ('baseline2', 'bn_bwd_reduce_kernel'), ('baseline2', 'bn_bwd_finalize_kernel'), ('baseline2', 'bn_bwd_dx_kernel')]


def _is(frag, name):
    return any(f in name for f in ((frag,) if isinstance(frag, str) else frag))


def card():
    import torch
    name = torch.cuda.get_device_name(0) or torch.cuda.get_device_properties(0).gcnArchName     # (a driver may report no name)
    try:
        out = subprocess.run(['rocm-smi', '--showuniqueid'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=30).stdout
        ids = [ln.split(':')[-1].strip() for ln in out.splitlines() if 'Unique ID' in ln and 'GPU[' in ln]
        idx = int(os.environ.get('HIP_VISIBLE_DEVICES', os.environ.get('ROCR_VISIBLE_DEVICES', '0')).split(',')[0] or 0)
        return '%s, unique id %s' % (name, ids[idx] if idx < len(ids) else (ids[0] if ids else 'unknown'))
    except Exception:  # noqa: BLE001
        return name


def run():
    import torch
    from sniper_amd import hip
    d = torch.device('cuda', 0)
    print('card: ' + card(), flush=True)
    for M, C in SHAPES:
        x = (torch.randn(M, C, device=d) * 1.5 + 0.3).half()
        dy, acc = torch.randn(M, C, device=d).half(), torch.randn(M, C, device=d).half()
        dx = torch.empty_like(x)
        gamma, beta = torch.rand(C, device=d) + 0.5, torch.randn(C, device=d) * 0.1
        mean, var = torch.randn(C, device=d) * 0.2 + 0.3, torch.rand(C, device=d) + 0.5
        sc, sh, inv = torch.empty(C, device=d), torch.empty(C, device=d), 1.0 / torch.sqrt(var + 2e-5)
        ws = torch.zeros(hip.query('sn_bn_workspace_bytes', M, C), dtype=torch.uint8, device=d)
        dg, db = torch.zeros(C, device=d), torch.zeros(C, device=d)
        st = hip.stream()
        hip.call('sn_bn_global_scale_shift', gamma, beta, mean, var, C, 2e-5, sc, sh, st)
        torch.cuda.synchronize()
        for _ in range(REPS):
            hip.call('sn_bn_backward', dy, x, acc, dx, M, C, C, C, C, C, sc, sh, mean, inv, 1, ws, dg, db, st)
            hip.call('sn_bn_frozen_backward', dy, x, acc, dx, M, C, C, C, C, C, sc, sh, mean, var, 2e-5, 1, ws, dg, db, st)
            hip.call('sn_bn_frozen_backward', dy, x, acc, dx, M, C, C, C, C, C, sc, sh, mean, var, 2e-5, 1, None, None, None, st)
            hip.call('sn_bn_frozen_backward', dy, x, None, None, M, C, C, C, C, C, sc, sh, mean, var, 2e-5, 1, ws, dg, db, st)
            hip.call('sn_bn_backward', dy, x, acc, dx, M, C, C, C, C, C, sc, sh, mean, inv, 1, ws, dg, db, st)
        torch.cuda.synchronize()
        print('shape %d x %d done' % (M, C), flush=True)


def report(root):
    files = glob.glob(os.path.join(root, '**', '*kernel_trace.csv'), recursive=True)
    assert files, 'no *kernel_trace.csv under ' + root
    rows = []
    for r in csv.DictReader(open(files[0])):
        name = r['Kernel_Name']
        if any(_is(frag, name) for _, frag in SEQ):
            rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), name))
    rows.sort()
    assert len(rows) == len(SHAPES) * REPS * len(SEQ), (len(rows), len(SHAPES) * REPS * len(SEQ))
    med = lambda v: sorted(v)[len(v) // 2]
    print('kernel time per call, us (median / min / max of %d repetitions after %d warm-up ones); bytes are the algorithmic ones:' % (REPS - WARM, WARM))
    print('baseline = sn_bn_backward, 12 B per element (reduce reads dy, x; dx reads dy, x, acc and writes dx); frozen = sn_bn_frozen_backward,')
    print('8 B per element (one pass); dx_only + par_only = the wide dx kernel (8 B) and the reduce-grid kernel (4 B) as two calls')
    k = 0
    for M, C in SHAPES:
        t = {}
        for rep in range(REPS):
            for variant, frag in SEQ:
                s, e, name = rows[k]
                k += 1
                assert _is(frag, name), (frag, name)
                if rep >= WARM:
                    t.setdefault(variant, {}).setdefault(rep, 0)
                    t[variant][rep] += e - s
        us = {v: [x / 1e3 for x in t[v].values()] for v in t}
        pair = [a + b for a, b in zip(us['dx_only'], us['par_only'])]
        base = us['baseline'] + us['baseline2']
        el = M * C
        line = '%6d x %4d  baseline %7.1f (%.1f - %.1f; %.2f TB/s)   frozen %7.1f (%.1f - %.1f; %.2f TB/s)   dx_only + par_only %7.1f (%.1f - %.1f)' % (
            M, C, med(base), min(base), max(base), 12 * el / med(base) / 1e6, med(us['frozen']), min(us['frozen']), max(us['frozen']),
            8 * el / med(us['frozen']) / 1e6, med(pair), min(pair), max(pair))
        print(line + '   frozen / baseline %.2f, pair / baseline %.2f; baseline first vs second call of a repetition %.1f / %.1f' % (
            med(us['frozen']) / med(base), med(pair) / med(base), med(us['baseline']), med(us['baseline2'])))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--report':
        report(sys.argv[2])
    else:
        run()
