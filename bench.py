"""bench.py -- SNIPER training throughput on MI355X (BASELINE.json metric: train chips/s, 512x512, R101).

    python bench.py --gpus N --steps K --warmup W          (N > 1: launched by torch.distributed.run)
    python bench.py ... --dump-outputs DIR                 (also writes what the last timed step computed: DIR/<name>.npy)
    python bench.py ... --full                             (also everything below "Extra objects")

A plain run sets up, warms up, times the K steps and prints one JSON line: the metric and the fields that say how it was
taken (config, device, graphs).  --full adds, after the timed steps, the measurements below; they run steps, passes and
processes of their own and leave the headline figure alone.

Workload (config.workload): BASELINE configs[1] -- ResNet-101 Faster-RCNN SNIPER, 3-scale chips,
20 x 512 x 512 chips per GPU, fp16 storage / fp32 accumulate, seeded synthetic COCO-shaped data
(sniper_amd/synthetic.py), random-init weights.  One *step* = one pass of the hot path over one chip
minibatch that is already resident in HBM: GPU anchor labelling of the 20 chips -> forward (conv
backbone, RPN, MultiProposalTarget, deformable PS-RoI pooling, heads, losses) -> backward -> gradient
all-reduce (RCCL, N > 1) -> multi-precision SGD update.  Every GPU owns an independent chip
minibatch (weak scaling, no sync-BN); value = N * B * K / max-over-ranks time.

NOT inside the step: the epoch chip database (chip generation / box assignment, a1-a4 of SURVEY section 8) and image
decoding / resizing -- they run once per epoch / ahead of the step and the chips are resident when the clock starts.

Extra objects on the JSON line (--full):
  roofline      the dominant kernel family (implicit-GEMM MFMA convolution: forward + data gradient + weight gradient
                launches) measured live with HIP events recorded on the stream each kernel is launched on, in extra untimed
                steps run eagerly (the timed region replays hipGraphs, inside which nothing can be bracketed):
                  achieved / frac        IN SITU: the kernels and the one stream of the timed step.  Sum of algorithmic FLOPs / sum of
                                         the launches' durations; this is the figure `rocprofv3 --kernel-trace --stats` of this
                                         command reproduces (tools/roofline_check.py, profiles/r03_roofline_check.json).
                  step_tflops            conv FLOPs of a step / the timed ms_per_step (end to end, everything else included).
                peak = 2.5 PFLOP/s dense fp16 MFMA (MI355X_MICROARCH.md).  traffic = HBM bytes per KERNEL launch of the family from
                rocprofv3 --pmc passes (traffic_detail: bytes per step, kernel launches per step), reported only when they were
                collected on THIS build of the convolution sources (else null); entry_calls_per_step counts C-ABI calls (one
                batched weight-gradient call covers up to 24 layers and several kernel launches).
                roofline_hbm = the memory-bound kernels of the step (RoI pooling, deformable sampling, BatchNorm, NMS, anchor
                labelling, SGD) against the 8 TB/s HBM roofline, from the same kind of PMC passes (profiles/pmc_kernels.json).
  cpu_baseline  the reference's CPU iterator path (chip extraction + box assignment + RPN anchor labelling) timed on this
                node's host cores on a bounded sample, chips/s: kind "reference" = the reference's own
                lib/data_utils/data_workers.py (lib2to3 artefact) over its compiled chips / bbox modules (oracle/_ref), kind
                "port" = the oracle/ restatement where that artefact is missing; it times the DATA PATH only and is a reported
                baseline, never a speed-up claim.  `c1` inside it:
                BASELINE configs[0] -- MobileNetV2 Faster-RCNN, 2 x 512 x 512 chips, one training step (forward + backward)
                through the reference-semantics CPU operators of oracle/graph_cpu.py.
  inference     BASELINE configs[4] (AutoFocus inference, `inf images/sec`) on injected FocusPixel maps (~10 % positive pixels in
                blobs), with its own cpu_baseline (the reference's aggregation + compiled soft-NMS under Pool(32));
                --no-inference skips it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0   # dense fp16, MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0


def conv_flops(name, a):
    """Algorithmic FLOPs of one conv-family launch from its C-ABI arguments."""
    if name in ('sn_conv_fwd', 'sn_conv_fwd_stats'):
        N, H, W, Cin, _, Cout, _, _, KH, KW, s, p, d = a[5:18]
    elif name in ('sn_conv_dgrad', 'sn_conv_dgrad_bn'):      # (the fused BatchNorm-backward variant has the same leading arguments)
        N, H, W, Cin, _, Cout, _, _, KH, KW, s, p, d = a[4:17]
    elif name == 'sn_conv_wgrad':
        N, H, W, Cin, _, Cout, _, KH, KW, s, p, d = a[3:15]
    elif name == 'sn_conv_wgrad_batch':          # a table of layers (sniper_amd.hip.wgrad_table), one launch per <= 24 of them
        tab, n = a[0], a[1]
        tot = 0.0
        for i in range(n):
            d = tab[i]
            Ho = (d.H + 2 * d.pad - d.dil * (d.KH - 1) - 1) // d.stride + 1
            Wo = (d.W + 2 * d.pad - d.dil * (d.KW - 1) - 1) // d.stride + 1
            tot += 2.0 * d.N * Ho * Wo * d.Cout * d.Cin * d.KH * d.KW
        return tot
    elif name == 'sn_conv_stem_fwd':
        N, Hp, Wp, Ho, Wo, Cout, _, KH, KWP, s = a[4:14]
        return 2.0 * N * Ho * Wo * Cout * KH * 7 * 3   # real 7x7x3 taps (the padded ones are zeros)
    else:
        return 0.0
    Ho = (H + 2 * p - d * (KH - 1) - 1) // s + 1
    Wo = (W + 2 * p - d * (KW - 1) - 1) // s + 1
    return 2.0 * N * Ho * Wo * Cout * Cin * KH * KW


def conv_shape(name, a):
    """(N, H, W, Cin, Cout, K, stride, dil) of a single-layer conv entry (forward: input dims; data gradient: dx dims), else None."""
    if name in ('sn_conv_fwd', 'sn_conv_fwd_stats'):
        N, H, W, Cin, _, Cout, _, _, KH, KW, s, p, d = a[5:18]
    elif name in ('sn_conv_dgrad', 'sn_conv_dgrad_bn'):
        N, H, W, Cin, _, Cout, _, _, KH, KW, s, p, d = a[4:17]
    else:
        return None
    return (int(N), int(H), int(W), int(Cin), int(Cout), int(KH), int(s), int(d))


class ConvProfiler(object):
    """Wraps sniper_amd.hip.call: brackets every conv-family launch with HIP events recorded on the
    stream the kernel is launched on (torch's current stream)."""
    NAMES = ('sn_conv_fwd', 'sn_conv_fwd_stats', 'sn_conv_dgrad', 'sn_conv_dgrad_bn', 'sn_conv_wgrad', 'sn_conv_wgrad_batch', 'sn_conv_stem_fwd')

    def __init__(self, extra=()):
        from sniper_amd import hip
        self.hip = hip
        self.orig = hip.call
        self.records = []
        self.extra = tuple(extra)           # further entry points to bracket (no FLOPs): name -> [calls, ms] in self.extra_ms
        self.extra_records = []

    def __enter__(self):
        def call(name, *args):
            if name in self.NAMES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = self.orig(name, *args)
                e1.record()
                self.records.append((name, conv_flops(name, args), e0, e1, conv_shape(name, args)))
                return r
            if name in self.extra:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = self.orig(name, *args)
                e1.record()
                self.extra_records.append((name, e0, e1))
                return r
            return self.orig(name, *args)
        self.hip.call = call
        import sniper_amd.engine.ops as ops
        import sniper_amd.engine.executor as ex
        self._mods = (ops, ex)
        return self

    def __exit__(self, *exc):
        self.hip.call = self.orig

    @staticmethod
    def bracket_overhead_ms(n=64):
        """What an EMPTY event bracket measures on this stream (event-to-event latency): subtracted from every launch's
        bracket so that the sum is the kernels' time, the quantity rocprofv3 --stats reports."""
        ev = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        v = sorted(a.elapsed_time(b) for a, b in ev)
        return v[len(v) // 2]

    def summary(self):
        torch.cuda.synchronize()
        over = self.bracket_overhead_ms()
        self.overhead_ms = over
        tot_ms, tot_fl, per = 0.0, 0.0, {}
        self.by_shape = {}
        for name, fl, e0, e1, shape in self.records:
            ms = max(e0.elapsed_time(e1) - over, 0.0)
            tot_ms += ms
            tot_fl += fl
            d = per.setdefault(name, [0, 0.0, 0.0])
            d[0] += 1
            d[1] += ms
            d[2] += fl
            if shape is not None:
                b = self.by_shape.setdefault((name,) + shape, [0, 0.0, 0.0])
                b[0] += 1
                b[1] += ms
                b[2] += fl
        self.extra_ms = {}
        for name, e0, e1 in self.extra_records:
            d = self.extra_ms.setdefault(name, [0, 0.0])
            d[0] += 1
            d[1] += max(e0.elapsed_time(e1) - over, 0.0)
        return tot_ms, tot_fl, per

    def shape_table(self, steps, top=28):
        """In-situ time per (entry, layer shape), largest first: which layers the family's time is in and at what rate."""
        rows = sorted(self.by_shape.items(), key=lambda kv: -kv[1][1])[:top]
        return [{'entry': k[0], 'shape': 'N%d %dx%d C%d->%d k%d s%d d%d' % k[1:], 'launches_per_step': v[0] // steps,
                 'us_per_launch': round(v[1] / v[0] * 1e3, 1), 'ms_per_step': round(v[1] / steps, 3),
                 'tflops': round(v[2] / (v[1] * 1e-3) / 1e12, 1) if v[1] > 0 else 0.0} for k, v in rows]


def device_identity(index=0):
    """Which physical card and at what clock: `unique_id` (the card's serial-like id: box-to-box spread of one build is 4-8 %, a
    reader must be able to tell spread from regression) and the current shader / memory clock levels from sysfs.  Best effort:
    empty fields where the node does not expose them."""
    import glob
    out = {'name': torch.cuda.get_device_name(index), 'unique_id': None, 'sclk_mhz': None, 'mclk_mhz': None}
    try:
        want = None
        try:
            props = torch.cuda.get_device_properties(index)
            bus = getattr(props, 'pci_bus_id', None)
            want = None if bus is None else '%02x:' % int(bus)
        except Exception:      # noqa: BLE001
            want = None
        cards = []
        for d in sorted(glob.glob('/sys/class/drm/card*/device')):
            if not os.path.exists(os.path.join(d, 'unique_id')) and not os.path.exists(os.path.join(d, 'pp_dpm_sclk')):
                continue
            slot = ''
            try:
                with open(os.path.join(d, 'uevent')) as fh:
                    for ln in fh:
                        if ln.startswith('PCI_SLOT_NAME='):
                            slot = ln.strip().split('=', 1)[1]
            except OSError:
                pass
            cards.append((d, slot))
        pick = [c for c in cards if want and want in c[1]] or cards
        if pick:
            d = pick[0][0]
            out['pci'] = pick[0][1]

            def level(fname):
                try:
                    with open(os.path.join(d, fname)) as fh:
                        for ln in fh:
                            if '*' in ln:
                                return int(''.join(ch for ch in ln.split(':', 1)[1] if ch.isdigit()))
                except (OSError, ValueError, IndexError):
                    return None
                return None
            try:
                with open(os.path.join(d, 'unique_id')) as fh:
                    out['unique_id'] = '0x' + fh.read().strip().lower().replace('0x', '')
            except OSError:
                pass
            out['sclk_mhz'], out['mclk_mhz'] = level('pp_dpm_sclk'), level('pp_dpm_mclk')
    except Exception as e:      # noqa: BLE001 -- identity is a report
        out['error'] = repr(e)
    return out


def conv_sources_hash():
    """Identity of the convolution kernels a PMC profile was collected on (the GPU box has no .git)."""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(ROOT, 'sniper_amd', 'csrc')
    for f in sorted(os.listdir(csrc)):
        if f.startswith('conv') and f.endswith(('.hip', '.h')):
            with open(os.path.join(csrc, f), 'rb') as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


def library_sources_hash():
    """Identity of the whole kernel library (every .hip / .h under csrc): what the per-kernel PMC report was collected on."""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(ROOT, 'sniper_amd', 'csrc')
    for f in sorted(os.listdir(csrc)):
        if f.endswith(('.hip', '.h')):
            with open(os.path.join(csrc, f), 'rb') as fh:
                h.update(fh.read())
    return h.hexdigest()[:16]


HBM_KERNELS = ('dpsroi_fwd_roi_kernel', 'dpsroi_bwd_data_mfma_kernel', 'dpsroi_bwd_trans_roi_kernel', 'deform_im2col_kernel',
               'deform_col2im_offset_kernel', 'deform_col2im_data_mfma_kernel', 'bn_apply_kernel', 'bn_bwd_dx_kernel',
               'bn_bwd_reduce_kernel', 'nms_lazy_kernel', 'topk_select_sort_kernel', 'anchor_finish_kernel', 'chips_generate_kernel',
               'sgd_dev', 'maxpool_kernel')


C4_HBM_KERNELS = ('psroi_ps_fwd', 'psroi_ps_bwd_data', 'psroi_ps_bwd_trans', 'avgpool_global')


INFER_HBM_KERNELS = ('topk_select_sort_kernel', 'nms_lazy_kernel', 'dpsroi_fwd_roi_kernel', 'bn_apply_kernel', 'deform_im2col_kernel',
                     'maxpool_kernel', 'im_prepare_kernel', 'splitk_reduce_kernel', 'det_compact', 'soft_nms_kernel',
                     '__amd_rocclr_copyBuffer', 'FillFunctor')


def roofline_hbm(path='pmc_kernels.json', names=None):
    """The memory-bound kernels of the step against the HBM roofline (8 TB/s): per kernel the launches, average duration and
    HBM bytes fetched / written per launch from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command
    (tools/gpu_session.sh pmc -> tools/pmc_report.py -> profiles/pmc_kernels.json; FETCH doubled, the gfx950 correction).  None
    unless that report was collected on THIS build of the kernel library."""
    try:
        with open(os.path.join(ROOT, 'profiles', path)) as fh:
            d = json.load(fh)
    except (OSError, ValueError):
        return None
    if d.get('library_sources_hash') != library_sources_hash():
        return None
    out = []
    for name in (names or HBM_KERNELS):
        # every kernel whose name contains `name` (the SGD update is a vec4 body kernel + a scalar head / tail kernel: one row,
        # launch-weighted), durations from the un-countered --stats run of the same command when the report has them (counter
        # collection slows a streaming kernel by ~50 %), else from the counter pass itself
        hit = [v for k, v in d.get('kernels', {}).items() if name in k]
        if not hit:
            continue
        n = sum(v['launches'] for v in hit)
        from_stats = all('avg_us_stats' in v for v in hit)
        us = sum(v['launches'] * (v['avg_us_stats'] if from_stats else v['avg_us']) for v in hit)
        fetch = sum(v['launches'] * v['fetch_bytes_per_launch'] for v in hit)
        write = sum(v['launches'] * v['write_bytes_per_launch'] for v in hit)
        gbs = round((fetch + write) / (us * 1e-6) / 1e9, 1) if us > 0 else None
        out.append({'kernel': name, 'kernels_matched': len(hit), 'launches_profiled': n, 'avg_us': round(us / n, 2),
                    'duration_from': 'kernel statistics run' if from_stats else 'counter pass',
                    'fetch_mb': round(fetch / n / 1e6, 2), 'write_mb': round(write / n / 1e6, 2),
                    'achieved_gb_s': gbs, 'frac_of_8tb_s': round(gbs / HBM_PEAK_GBS, 3) if gbs else None})
    return out or None


def pmc_traffic():
    """HBM bytes per conv-family launch from the committed rocprofv3 --pmc passes of this same command
    (tools/pmc_traffic.py -> profiles/pmc_traffic.json; FETCH_SIZE / WRITE_SIZE in separate passes, FETCH doubled
    as MI355X_MICROARCH.md section HBM prescribes for gfx950).  None when no profile exists FOR THIS BUILD of the
    convolution sources: a stale constant is not a measurement."""
    path = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')
    try:
        with open(path) as fh:
            d = json.load(fh)
        if d.get('conv_sources_hash') != conv_sources_hash():
            return None
        pmc_traffic.detail = {k: d.get(k) for k in ('hbm_bytes_per_step', 'kernel_launches_per_step', 'launches', 'steps')}
        return d.get('hbm_bytes_per_launch')
    except (OSError, ValueError):
        return None


def cpu_baseline(seconds_target=15.0):
    """The reference's CPU data path, Pool(P) over images like MNIteratorE2E does.  kind "reference": the reference's OWN
    lib/data_utils/data_workers.py (chip_worker.chip_extractor / box_assigner, anchor_worker.worker) over its compiled chips /
    bbox modules -- the lib2to3 artefact and the modules oracle/build.py made from the reference sources (oracle/_ref, present on
    the GPU box); kind "port": oracle/data_path.py, the restatement pinned against them, where the artefact is missing."""
    import multiprocessing as mp
    from oracle import build as obuild
    from oracle import ref_py
    use_ref = ref_py.available() and os.environ.get('SNIPER_CPU_BASELINE', 'reference') != 'port'
    if not use_ref:
        obuild.build_restatement()
    fn = _cpu_image_chips_ref if use_ref else _cpu_image_chips
    # BASELINE.md section 3 / SURVEY 8(d): P = os.cpu_count() of the benchmark node, P printed (until round 5: min(cores, 64), the
    # reference config's TRAIN.NUM_PROCESS; SNIPER_CPU_BASELINE_PROCS restores any other pool size)
    P = int(os.environ.get('SNIPER_CPU_BASELINE_PROCS', 0)) or (os.cpu_count() or 1)
    with mp.get_context('fork').Pool(P) as pool:
        pool.map(fn, range(P), chunksize=1)          # warm the workers (imports, anchor tables)
        # bounded sample: a pilot batch sizes the timed batch to about `seconds_target` of wall time
        t0 = time.time()
        pool.map(fn, range(8 * P), chunksize=4)
        pilot = max(time.time() - t0, 1e-3)
        n_img = int(min(max(8 * P * seconds_target / pilot, 8 * P), 4096 * P))
        t0 = time.time()
        chips = pool.map(fn, range(10 ** 6, 10 ** 6 + n_img), chunksize=4)
        dt = time.time() - t0
    n_chips = int(sum(chips))
    what = ('the reference\'s own chip_worker.chip_extractor + box_assigner + anchor_worker.worker (lib/data_utils/data_workers.py '
            'translated by lib2to3, over its compiled chips.pyx / cchips.cpp / bbox.pyx; oracle/_ref)' if use_ref else
            'chip_extractor + box_assigner + anchor_worker (oracle/data_path.py, restating lib/data_utils/data_workers.py)')
    return {'value': n_chips / dt, 'unit': 'chips/s', 'cores': P, 'node_cores': os.cpu_count(),      # cores = the pool the work ran on
            'kind': 'reference' if use_ref else 'port',
            'scope': 'data path only (a3-a6 of SURVEY section 8): a reported baseline, not comparable with the training-step '
                     'throughput above',
            'sample': '%d synthetic images -> %d chips: %s under multiprocessing.Pool(%d), %.1f s' % (n_img, n_chips, what, P, dt)}


def cpu_c1_step():
    """BASELINE configs[0]: MobileNetV2 Faster-RCNN, 1 scale, 2 x 512 x 512 synthetic chips through reference-semantics CPU
    operators (oracle/graph_cpu.py: torch-CPU fp32 for the standard operators, oracle/nn.py for the fork-resident ones) --
    one training step, forward + backward.  (MXNet-CPU itself cannot be installed here: SURVEY section 8(d).)"""
    from oracle import graph_cpu
    from sniper_amd import config as cfgmod
    from sniper_amd.symbols.faster import mobilenetv2_e2e as mn
    B, A, F = 2, 15, 16
    cfg = cfgmod.mobilenetv2_e2e(batch_images=B)
    sym = mn.mobilenetv2_e2e().get_symbol_rcnn(cfg)
    shapes = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, A * F * F),
                  bbox_target=(B, 4 * A, F, F), bbox_weight=(B, 4 * A, F, F), gt_boxes=(B, 100, 5), crowd_boxes=(B, 10, 5))
    rs = np.random.RandomState(11)
    args, _, auxs = sym.infer_shape(**shapes)
    P, AUX = {}, {}
    for name, shp in zip(sym.list_arguments(), args):
        if name in shapes:
            continue
        if name.endswith('_gamma'):
            P[name] = rs.uniform(0.5, 0.9, shp).astype(np.float32)
        elif name.endswith(('_beta', '_bias')):
            P[name] = np.zeros(shp, np.float32)
        else:
            P[name] = (rs.standard_normal(shp) * (0.01 if name.startswith(('rpn_', 'fc_', 'cls_', 'bbox_')) else
                                                  np.sqrt(2.0 / np.prod(shp[1:])))).astype(np.float32)
    for name, shp in zip(sym.list_auxiliary_states(), auxs):
        AUX[name] = np.ones(shp, np.float32) if name.endswith('_var') else np.zeros(shp, np.float32)
    gt = -np.ones((B, 100, 5), np.float32)
    for b in range(B):
        c, wh = rs.uniform(60, 450, (40, 2)), rs.uniform(40, 320, (40, 2))
        gt[b, :40, :4] = np.clip(np.concatenate((c - wh / 2, c + wh / 2), 1), 0, 511)
        gt[b, :40, 4] = rs.randint(1, 81, 40)
    inp = dict(data=(rs.standard_normal((B, 3, 512, 512)) * 50).astype(np.float32), valid_ranges=np.array([[0, 512]] * B, np.float32),
               im_info=np.array([[512, 512, 1.0]] * B, np.float32),
               label=rs.choice([-1, 0, 1], size=(B, A * F * F), p=[0.9, 0.07, 0.03]).astype(np.float32),
               bbox_target=(rs.standard_normal((B, 4 * A, F, F)) * 0.3).astype(np.float32),
               bbox_weight=(rs.uniform(size=(B, 4 * A, F, F)) < 0.05).astype(np.float32), gt_boxes=gt,
               crowd_boxes=-np.ones((B, 10, 5), np.float32))
    t0 = time.time()
    outs, _ = graph_cpu.run(sym, P, AUX, inp)
    dt = time.time() - t0
    assert all(np.isfinite(o).all() for o in outs)
    return {'metric': 'train chips/sec (512x512, MobileNetV2, CPU)', 'value': round(B / dt, 3), 'unit': 'chips/s',
            'seconds_per_step': round(dt, 2), 'cores': int(torch.get_num_threads()), 'kind': 'port',
            'sample': 'BASELINE configs[0]: 1 training step (forward + backward) of MobileNetV2 Faster-RCNN on 2 x 512 x 512 synthetic '
                      'chips through oracle/graph_cpu.py (torch-CPU fp32 + oracle/nn.py), %d torch threads' % torch.get_num_threads()}


def _cpu_image_chips(i):
    from oracle import data_path
    from sniper_amd import config as cfgmod
    from sniper_amd.synthetic import make_roidb
    cfg = cfgmod.res101_e2e()
    r = make_roidb(1, seed=100000 + i, n_proposals=0)[0]
    np.random.seed(i)
    crops = data_path.chip_extractor(r, cfg.TRAIN.SCALES, cfg.TRAIN.VALID_RANGES, 512, 56, None)
    r['crops'] = crops
    props = data_path.box_assigner(r, cfg.TRAIN.SCALES, cfg.TRAIN.VALID_RANGES, 512, 56, False, None)[0]
    at = _cpu_image_chips.at = getattr(_cpu_image_chips, 'at', None) or data_path.AnchorTarget(
        512, 16, cfg.network.ANCHOR_RATIOS, cfg.network.ANCHOR_SCALES)
    gtids = np.where(r['max_overlaps'] == 1)[0]
    for ci, crop in enumerate(crops):
        at([512, 512, crop[1]], crop[0].copy(), crop[1], props[ci], gtids, r['boxes'][gtids].copy(), r['boxes'].copy(),
           r['max_classes'][gtids].reshape(-1, 1))
    return len(crops)


def _cpu_image_chips_ref(i):
    """one image through the reference's own workers (oracle/ref_py.py loads them; per-process cache on the function)"""
    from oracle import ref_py
    from sniper_amd import config as cfgmod
    from sniper_amd.synthetic import make_roidb
    st = getattr(_cpu_image_chips_ref, 'st', None)
    if st is None:
        ns = ref_py.load()
        cfg = cfgmod.res101_e2e()
        np.random.seed(0)
        cw = ns.data_workers.chip_worker(cfg, 512)
        cw.chip_stride = 56
        cw.chip_generator = ns.chip_generator.chip_generator(chip_stride=56, use_cpp=True)
        aw = ns.data_workers.anchor_worker(cfg, 512)
        st = _cpu_image_chips_ref.st = (cw, aw)
    cw, aw = st
    r = make_roidb(1, seed=100000 + i, n_proposals=0)[0]
    np.random.seed(i)
    ref_py.srand(i)
    crops = cw.chip_extractor(r)
    r['crops'] = crops
    props = cw.box_assigner(r)[0]
    gtids = np.where(r['max_overlaps'] == 1)[0]
    for ci, crop in enumerate(crops):
        aw.worker([[512, 512, crop[1]], crop[0].copy(), crop[1], props[ci], gtids, r['boxes'][gtids].copy(), r['boxes'].copy(),
                   r['max_classes'][gtids].reshape(-1, 1)])
    return len(crops)


def focus_map_blobs(scale_i, image, chip, net_map, frac=0.10):
    """Synthetic FocusPixel map of the network map's shape (2, h, w): ~`frac` of the pixels positive, in 2-4 round blobs
    (what a trained AutoFocus branch marks -- regions that contain small objects; a random-init branch marks nearly
    everything, so every image would stay one full-size chip at every scale and FocusChip generation, chip batching and area-sorted
    padding would never run).  Deterministic in (scale, image, chip)."""
    _, h, w = net_map.shape
    rs = np.random.RandomState(1000003 * scale_i + 1009 * image + chip)
    k = int(rs.randint(2, 5))
    r = np.sqrt(frac * h * w / (k * np.pi))
    yy, xx = np.mgrid[0:h, 0:w]
    pos = np.zeros((h, w), bool)
    for b in range(k):       # one blob per stratum of the longer side (objects of a scene are spread out, not stacked), jittered
        u, v = (b + 0.5 + rs.uniform(-0.2, 0.2)) / k, rs.uniform(0.2, 0.8)
        cx, cy = (u * w, v * h) if w >= h else (v * w, u * h)
        pos |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    out = np.empty((2, h, w), np.float32)
    out[1] = np.where(pos, 0.9, 0.02)
    out[0] = 1.0 - out[1]
    return out


def bench_inference(passes=5, jobs=None):
    """BASELINE config C5: ResNet-101 AutoFocus inference, 3-scale coarse-to-fine FocusChip pyramid
    ((480,512) -> (800,1280) -> (1400,2000), batches of 8 / 8 / 2), 64 synthetic 640x480 images per pass, random-init weights, the
    FocusPixel maps that drive the chip generation injected (focus_map_blobs: ~10 % positive pixels in blobs).
    One pass = GPU image preparation + forward + box decoding + score threshold / border pruning (sn_det_compact) + FocusChips +
    multi-scale soft-NMS aggregation; batches of a scale run on up to three lanes (streams) and the host slices a batch's rows
    under the following forwards (Tester.get_detections).
    Throughput of the last pass (bound executors cached per batch shape and replaying their captured forward, like a resident
    service: pass 1 binds, pass 2 captures, passes 3.. replay).  `single_batch_pass`: the first 8 images as a pass of their own,
    the number of rounds 2-4.  cpu_baseline: the reference's aggregation of the SAME per-scale detections on the host -- its loops
    + its compiled cpu_soft_nms under Pool(32) (oracle/inference_ref.py)."""
    import multiprocessing as mp
    import sniper_amd.mx as mx
    from sniper_amd import config as cfgmod
    from sniper_amd.inference import imdb_detection_wrapper
    from sniper_amd.symbols.faster import resnet_mx_101_e2e as rn

    class Imdb(object):
        num_classes, classes, name, result_path = 81, None, 'synthetic', None
    rs = np.random.RandomState(0)
    n_long, n_short = 64, 8
    images = [{'image': rs.randint(0, 256, (480, 640, 3)).astype(np.uint8), 'width': 640, 'height': 480, 'flipped': False,
               'gt_overlaps': np.zeros((1, 81), np.float32)} for _ in range(n_long)]
    cfg = cfgmod.res101_e2e_autofocus()
    # TEST.CONCURRENT_JOBS (yml: 2 model processes per GPU) stays 1: the wrapper's thread-per-job form of it measured slower than
    # one thread driving `lanes` streams (84-89 vs 96-103 images/s, host-side contention); the lanes are this engine's way to keep
    # several small batches in flight
    jobs = 1 if jobs is None else jobs
    lanes = 3
    cache, blobs = {}, {}

    def fmap(scale_i, image, chip, net_map):
        # the synthetic stand-in for the network's map is an INPUT of the pass, deterministic in (scale, image, chip): drawn
        # once, not re-drawn inside every timed pass
        key = (scale_i, image, chip, tuple(net_map.shape))
        if key not in blobs:
            blobs[key] = focus_map_blobs(scale_i, image, chip, net_map)
        return blobs[key]

    def one_pass(base, scale_dets=False):
        roidb = [dict(r) for r in base]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = imdb_detection_wrapper(rn.resnet_mx_101_e2e, cfg, Imdb(), roidb, [mx.gpu(0)], None, None, module_cache=cache,
                                     focus_map_fn=fmap, return_scale_dets=scale_dets, concurrent_jobs=jobs, lanes=lanes)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    def run(base, n_passes):
        # the timed passes are the product's default path: every chip's rows stay in HBM, aggregation on the device, one copy of the
        # final boxes (Tester.aggregate_device); one more pass, untimed, brings the per-scale detection lists to the host for the
        # chip counts and the CPU baseline of the aggregation
        dt = None
        for _ in range(n_passes):
            dt, _ = one_pass(base)
        _, (_, dets) = one_pass(base, scale_dets=True)
        # chips per image at every scale: scale 0 is the whole image; the per-scale detection lists record how many chips ran
        chips_by_scale = [[len(d[1][i]) for i in range(len(base))] for d in dets]
        return dt, dets, chips_by_scale

    def bound_executors():
        mods = [m for k, m in cache.items() if hasattr(m, '_exes')] + \
               [m for k, v in cache.items() if isinstance(k, tuple) and k and k[0] == '__lanes__' for m in v]
        return sum(len(m._exes) for m in mods)
    # one batch of 8 images (rounds 2-4 reported this pass as the value; kept beside it): 1 + 1 + ~9 batches, and between the
    # scales the host phases nothing overlaps -- collect, FocusChips, new iterator, first image preparation: ~10 ms of its 44
    sdt, _, schips = run(images[:n_short], passes)
    # the pass the value is quoted on: 64 images = 8 batches of 8 at the coarsest scale (BASELINE configs[4]: "batch 8 images";
    # the reference walks a 5000-image roidb per pass, lib/inference.py:439-529)
    base = images
    dt, dets, chips_by_scale = run(base, passes)
    total_chips = [int(sum(c)) for c in chips_by_scale]
    # `value`: the configuration the metric is quoted on (8 synthetic 640x480 images, batch 8) -- one batch at the coarsest
    # scale; `value_steady`: 64 images per pass (8 batches of 8: the per-scale host phases amortised, as over a roidb)
    out = {'metric': 'inf images/sec', 'value': round(n_short / sdt, 2), 'unit': 'images/s', 'seconds_per_pass': round(sdt, 3),
           'images': n_short, 'value_steady': round(len(base) / dt, 2), 'images_steady': len(base), 'seconds_per_pass_steady': round(dt, 3),
           'chips_by_scale': total_chips, 'chips_per_image_by_scale': [round(c / float(len(base)), 2) for c in total_chips],
           'concurrent_jobs': jobs, 'lanes': lanes,
           'workload': 'ResNet-101 AutoFocus inference, 3-scale FocusChip pyramid (480,512) -> (800,1280) -> (1400,2000), batches of '
                       '8 / 8 / 2 chips (BASELINE configs[4]); %d synthetic 640x480 images per pass, random-init weights; FocusPixel '
                       'maps injected: ~10 %% positive pixels in 2-4 blobs per chip (SURVEY 8(d)) -> FocusChips at the finer '
                       'scales as counted; up to %d batches of a scale in flight on their own HIP streams (lanes), score '
                       'threshold + border pruning on the GPU, host slicing of batch b under the forwards of the following '
                       'batches' % (len(base), lanes),
           'single_batch_pass': {'images': n_short, 'value': round(n_short / sdt, 2), 'unit': 'images/s', 'seconds_per_pass': round(sdt, 3),
                                 'chips_per_image_by_scale': schips,
                                 'what': 'the first %d of the images as a pass of their own -- the pass rounds 2-4 quoted (96, 160 - 175, '
                                         '170 - 180 images/s): one batch at the coarsest scale, so the per-scale host phases '
                                         '(collect, FocusChips, iterator, first image preparation) are not amortised' % n_short}}
    # ---- what a batch shape the service has NOT met costs: 32 images of the other COCO aspect ratios of the
    # SURVEY 8(d) roidb through the same warm Modules -- their chips land in (H/64, W/64) buckets the passes above never bound.
    # Pass 1 binds them and (since the first-forward capture of round 6, Module._exe_for: capture_first) captures their hipGraphs, pass 2
    # meets the (shape, lane) pairs pass 1 left, pass 3 replays: cold_shape_ms = the extra time of passes 1 and 2 over pass 3 per newly
    # bound executor; value_unseen_shapes = images/s of pass 1 (every shape new; until round 5 that pass ran eagerly and pass 2 captured).
    try:
        sizes = [(480, 640), (427, 640), (375, 500), (640, 427)]             # (h, w): not the 640 x 480 of the passes above
        rs2 = np.random.RandomState(1)
        odd = [{'image': rs2.randint(0, 256, (h, w, 3)).astype(np.uint8), 'width': w, 'height': h, 'flipped': False,
                'gt_overlaps': np.zeros((1, 81), np.float32)} for h, w in (sizes[i % len(sizes)] for i in range(32))]
        e0 = bound_executors()
        t1, _ = one_pass(odd)
        t2, _ = one_pass(odd)
        t3, _ = one_pass(odd)
        new = bound_executors() - e0
        out['unseen_shapes'] = {'images': len(odd), 'new_executors': new, 'seconds_pass1_bind': round(t1, 3),
                                'seconds_pass2_capture': round(t2, 3), 'seconds_pass3_replay': round(t3, 3),
                                'capture_first': os.environ.get('SNIPER_CAPTURE_FIRST', '1') != '0'}
        out['value_unseen_shapes'] = round(len(odd) / t1, 2)
        out['cold_shape_ms'] = round(((t1 - t3) + (t2 - t3)) / max(new, 1) * 1e3, 1)
    except Exception as e:      # noqa: BLE001 -- a report
        out['unseen_shapes'] = {'failed': repr(e)}
    # ---- roofline of the pass (untimed, after the measurement): one more pass on ONE lane with the executors running eagerly
    # (a replayed hipGraph cannot be bracketed), every conv-family entry and the other device entries of the pass between HIP
    # events on their stream.  FLOPs from the entries' arguments (as the training roofline), so it is what these chips cost.
    try:
        os.environ['SNIPER_HIP_GRAPHS'] = '0'
        cache.clear()                 # (the timed passes' Modules: their pools and graphs go at the next bind, Module.bind -> thaw_heap)
        cache2 = {}
        extra = ('sn_multi_proposal', 'sn_dpsroi_pool_fwd', 'sn_deform_im2col', 'sn_bn_apply', 'sn_bbox_decode', 'sn_det_compact',
                 'sn_soft_nms_batch', 'sn_im_prepare', 'sn_maxpool_fwd', 'sn_softmax_fwd', 'sn_transpose_batched', 'sn_copy2d')
        res = None
        for rep in range(2):                 # the first pass binds (allocations, parameter packing), the second is measured
            roidb = [dict(r) for r in base]
            with ConvProfiler(extra=extra) as prof:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                imdb_detection_wrapper(rn.resnet_mx_101_e2e, cfg, Imdb(), roidb, [mx.gpu(0)], None, None, module_cache=cache2,
                                       focus_map_fn=fmap, concurrent_jobs=1, lanes=1)
                torch.cuda.synchronize()
                eager_dt = time.perf_counter() - t0
                res = prof.summary()
                extra_ms, table = prof.extra_ms, prof.shape_table(1, top=12)
        tot_ms, tot_fl, per = res
        tf = tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0
        out['roofline'] = {
            'bound': 'mfma', 'kernel': 'conv_dma_kernel / conv_igemm_kernel through sn_conv_fwd (BatchNorm folded), sn_conv_stem_fwd',
            'achieved': round(tf, 1), 'peak': MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(tf / MFMA_PEAK_TFLOPS, 4),
            'gflop_per_pass': round(tot_fl / 1e9, 1), 'gflop_per_image': round(tot_fl / 1e9 / len(base), 1),
            'conv_ms_per_pass': round(tot_ms, 2), 'conv_launches_per_pass': sum(v[0] for v in per.values()),
            'pass_tflops': round(tot_fl / dt / 1e12, 1),      # conv FLOPs of a pass / the TIMED seconds per pass (end to end)
            'mode': 'one extra pass, one lane, executors eager, HIP events around every entry on its stream (sum of launch '
                    'durations; the timed passes replay hipGraphs on %d lanes)' % lanes,
            'eager_seconds_per_pass': round(eager_dt, 3),
            'other_entries_ms_per_pass': {k: {'calls': v[0], 'ms': round(v[1], 3)} for k, v in sorted(extra_ms.items(), key=lambda kv: -kv[1][1])},
            'by_shape': table,
            # the memory-bound kernels of the pass against 8 TB/s: bytes per launch from the committed FETCH_SIZE / WRITE_SIZE passes
            # of a 16-image pass on THIS build (tools/gpu_session.sh pmcinf -> profiles/pmc_infer_kernels.json); None otherwise
            'roofline_hbm': roofline_hbm('pmc_infer_kernels.json', INFER_HBM_KERNELS),
            'note': 'batches of 8 / 8 / 2 chips: most launches are a small fraction of a wave of tiles, so the conv family runs '
                    'far below the training step\'s rate; see DESIGN.md'}
    except Exception as e:      # noqa: BLE001 -- a report
        out['roofline'] = {'failed': repr(e)}
    finally:
        os.environ.pop('SNIPER_HIP_GRAPHS', None)
    try:
        from oracle import inference_ref
        P = min(os.cpu_count() or 1, 32)             # Pool(32): lib/inference.py:159
        with mp.get_context('fork').Pool(P) as pool:
            inference_ref.aggregate(dets, cfg.TEST.VALID_RANGES, len(base), 81, cfg.TEST.NMS_SIGMA, pool)      # warm the workers
            reps, t0 = 0, time.perf_counter()
            while reps < 3 or time.perf_counter() - t0 < 3.0:
                inference_ref.aggregate(dets, cfg.TEST.VALID_RANGES, len(base), 81, cfg.TEST.NMS_SIGMA, pool)
                reps += 1
            cdt = (time.perf_counter() - t0) / reps
        n_boxes = int(sum(len(d[j][i][c]) for d in dets for j in range(1, 81) for i in range(len(base)) for c in range(len(d[j][i]))))
        out['cpu_baseline'] = {
            'value': round(len(base) / cdt, 2), 'unit': 'images/s', 'cores': P, 'node_cores': os.cpu_count(), 'kind': inference_ref.kind(),
            'scope': 'post-processing leg only (multi-scale aggregation + soft-NMS of the %d (image, class) problems, %d candidate '
                     'boxes); the forward passes have no CPU counterpart here (no MXNet)' % (len(base) * 80, n_boxes),
            'sample': 'the reference\'s Tester.aggregate loops (lib/inference.py:166-201) + its compiled cpu_soft_nms '
                      '(lib/nms/cpu_nms.pyx) under multiprocessing.Pool(%d) on this pass\'s per-scale detections, %d repetitions, '
                      '%.3f s each' % (P, reps, cdt)}
    except Exception as e:      # noqa: BLE001 -- a baseline is a report
        out['cpu_baseline'] = {'value': None, 'sample': 'failed: %r' % (e,)}
    return out


def dist_probe(tr, step, sync, dist, world, reps=3):
    """N > 1 only, untimed extra steps on EVERY rank (collectives): what the gradient exchange costs and how much of it the split
    backward hides.
      allreduce_ms      the whole gradient arena summed over the ranks, alone on an idle device (fp16 + fp32 buckets as in a step)
      overlap_frac      of the first segment's collective (gradients of the steps behind the split), the part that ran under the
                        second backward segment: |[comm start, comm end] intersect [segment-2 start, segment-2 end]| / comm
                        duration, from HIP events on the two streams (comm start = segment-2 start: the collective is released
                        by the event that ends segment 1)
      rccl_ranks_seen   sum over the ranks of 1 through the process group (= world when every rank took part)"""
    import sniper_amd.parallel as par
    mod, ex = tr.mod, tr.mod.exe
    ones = torch.ones(1, device='cuda')
    dist.all_reduce(ones)
    ranges = [(h, a, b) for _, h, a, b in ex.ar_ranges]
    half = mod._half_buf()
    par.allreduce_ranges(ex.grad_arena(), ranges, dist, half)                  # warm (communicator set-up)
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    n_coll = 0
    for _ in range(reps):
        n_coll = par.allreduce_ranges(ex.grad_arena(), ranges, dist, half)
    e1.record()
    sync()
    ar_ms = e0.elapsed_time(e1) / reps
    nbytes = sum((b - a) * (2 if (h and os.environ.get('SNIPER_GRAD_FP16', '1') != '0') else 4) for h, a, b in ranges)
    rep = {'backend': dist.get_backend(), 'rccl_ranks_seen': int(round(float(ones.item()))), 'allreduce_ms': round(ar_ms, 3),
           'allreduce_mb': round(nbytes / 1e6, 1), 'collectives_per_step': n_coll,
           'allreduce_gb_s_algorithmic': round(nbytes / (ar_ms * 1e-3) / 1e9, 1) if ar_ms > 0 else None,
           'split_backward': bool(ex.split_k), 'overlap_frac': None, 'first_segment_ms': None}
    if ex.split_k:
        mod._comm_probe = []
        try:
            for i in range(reps):
                step(i)
            sync()
            fr, ms = [], []
            for p in mod._comm_probe:
                if 'seg2_end' not in p:
                    continue
                comm = p['seg2_start'].elapsed_time(p['comm_end'])
                seg2 = p['seg2_start'].elapsed_time(p['seg2_end'])
                if comm > 0:
                    fr.append(max(0.0, min(comm, seg2)) / comm)
                    ms.append(comm)
            if fr:
                rep['overlap_frac'] = round(sum(fr) / len(fr), 3)
                rep['first_segment_ms'] = round(sum(ms) / len(ms), 3)
        finally:
            mod._comm_probe = None
    t = torch.tensor([rep['allreduce_ms']], device='cuda', dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)                                   # the slowest rank's exchange (overlap_frac: rank 0's)
    rep['allreduce_ms'] = round(float(t[0].item()), 3)
    return rep


LINE_LIMIT = 4096      # bytes of the final JSON line (the driver keeps a tail of about 8 KB of stdout)
DUMP_LIMIT = 64 << 20  # bytes of all arrays --dump-outputs writes
PARAM_SAMPLE = 1024    # elements per parameter tensor in params_sample.npy


def dump_outputs(path, lab, outs, output_names, arg_params):
    """--dump-outputs: what the last timed step computed, as <name>.npy (floating point as float32, integers as float64,
    both exact) -- the anchor labelling results (label_*), the network outputs (out_*) and, for the backward pass and the
    SGD update, a fixed sample of the updated parameters (params_sample: per parameter in name order, PARAM_SAMPLE elements
    drawn by a generator seeded from the name).  An array past the DUMP_LIMIT budget is replaced by a seeded sample of its
    elements (<name>_sample).  Returns {file name: shape}."""
    import re
    import zlib

    def seeded(name):
        return np.random.default_rng(zlib.crc32(name.encode()))

    arrays = [('label_' + k, v) for k, v in sorted(lab.items())]
    arrays += [('out_' + n, o) for n, o in zip(output_names, outs)]
    sample = []
    for name in sorted(arg_params):
        p = np.asarray(arg_params[name].asnumpy(), np.float32).reshape(-1)
        idx = np.sort(seeded(name).choice(p.size, min(p.size, PARAM_SAMPLE), replace=False))
        sample.append(p[idx])
    arrays.append(('params_sample', np.concatenate(sample)))
    os.makedirs(path, exist_ok=True)
    left, written = DUMP_LIMIT, {}
    for name, a in arrays:
        a = a.asnumpy() if hasattr(a, 'asnumpy') else a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        a = a.astype(np.float32 if a.dtype.kind == 'f' else np.float64)
        name = re.sub(r'[^A-Za-z0-9_.-]', '_', name)
        if a.nbytes > left:
            idx = np.sort(seeded(name).choice(a.size, left // a.itemsize, replace=False))
            a, name = a.reshape(-1)[idx], name + '_sample'
        np.save(os.path.join(path, name + '.npy'), a)
        left -= a.nbytes
        written[name] = list(a.shape)
    return written


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact_line(full):
    """The ONE final line: the contract's fields + roofline + cpu_baseline + the inference leg's headline, nothing that grows with
    the number of layer shapes or kernels.  Whatever a later edit adds to the full record stays off this line unless named here;
    if the line still exceeds LINE_LIMIT the optional groups are dropped last-first (never the contract's fields)."""
    line = _pick(full, ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                        'vs_baseline', 'dtype', 'data', 'graphs'))
    line['vs_baseline'] = full.get('vs_baseline')
    cfg = full.get('config') or {}
    line['config'] = {'workload': 'ResNet-101 Faster-RCNN SNIPER 3-scale, batch %s x 512x512 fp16 per GPU (BASELINE configs[1]); step = '
                                  'anchor labelling + fwd + bwd + all-reduce + SGD on HBM-resident chips' % cfg.get('chips_per_gpu'),
                      'chips_per_gpu': cfg.get('chips_per_gpu'), 'global_batch': cfg.get('global_batch'), 'parallelism': cfg.get('parallelism')}
    line['device'] = _pick(full.get('device') or {}, ('name', 'unique_id', 'sclk_mhz', 'mclk_mhz'))
    roof = full.get('roofline') or {}
    r = _pick(roof, ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'gflop_per_step', 'conv_ms_per_step', 'step_tflops',
                     'entry_calls_per_step'))
    r['traffic'] = roof.get('traffic')
    r['traffic_bytes_per_launch'] = roof.get('traffic')      # (the same number under the name that says what it is: VERDICT r5 weak #12)
    r['traffic_unit'] = 'HBM bytes per kernel LAUNCH of the family (rocprofv3 PMC passes); per step: traffic_bytes_per_step'
    r['kernel'] = 'conv_dma_kernel / wgrad_ps_kernel family (implicit-GEMM MFMA convolution: fwd + dgrad + wgrad)'
    xc = roof.get('rocprof_cross_check') or {}
    if xc.get('frac_rocprof') is not None:
        r['rocprof_frac'] = xc['frac_rocprof']
    td = roof.get('traffic_detail') or {}
    if td.get('hbm_bytes_per_step') is not None:
        r['traffic_bytes_per_step'] = td['hbm_bytes_per_step']
    line['roofline'] = r
    cpu = full.get('cpu_baseline')
    if isinstance(cpu, dict):
        c = _pick(cpu, ('value', 'unit', 'cores', 'node_cores', 'kind'))
        if c.get('value') is not None:
            c['value'] = round(c['value'], 1)
        c['sample'] = str(cpu.get('sample', ''))[:160]
        if isinstance(cpu.get('c1'), dict) and cpu['c1'].get('value') is not None:
            c['c1_mnv2_chips_s'] = cpu['c1']['value']
        line['cpu_baseline'] = c
    else:
        line['cpu_baseline'] = None
    if isinstance(full.get('c4'), dict):      # BASELINE configs[3] at one GPU's share: three numbers
        line['c4'] = _pick(full['c4'], ('value', 'unit', 'ms_per_step', 'head_ms', 'chips_per_gpu'))
    for k in ('dist', 'fit_path'):
        if isinstance(full.get(k), dict):
            line[k] = {a: b for a, b in full[k].items() if not isinstance(b, (dict, list, str)) or (isinstance(b, str) and len(b) <= 80)}
    inf = full.get('inference')
    if isinstance(inf, dict):
        i = _pick(inf, ('metric', 'value', 'unit', 'images', 'seconds_per_pass', 'value_steady', 'images_steady', 'seconds_per_pass_steady',
                        'cold_shape_ms', 'value_unseen_shapes', 'lanes'))
        if isinstance(inf.get('roofline'), dict):
            i['roofline'] = _pick(inf['roofline'], ('bound', 'achieved', 'peak', 'unit', 'frac', 'pass_tflops'))
        if isinstance(inf.get('cpu_baseline'), dict):
            i['cpu_baseline'] = _pick(inf['cpu_baseline'], ('value', 'unit', 'cores', 'kind'))
        line['inference'] = i
    line['detail'] = 'BENCH_DETAIL line above / gpurun_out/bench_detail.json'
    for drop in ('detail', 'fit_path', 'c4', 'dist', 'device', 'inference'):
        if len(json.dumps(line)) < LINE_LIMIT:
            break
        line.pop(drop, None)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=20, help='chips per GPU (BASELINE C2: 20)')
    ap.add_argument('--full', action='store_true', help='after the timed steps also measure the conv roofline, the host cost of a '
                    'step, the CPU baselines, BASELINE configs C4 and C5, fit_path and (N > 1) the all-reduce; print the full record')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='(--full) skip the CPU baselines')
    ap.add_argument('--inference', action='store_true', help='(--full: default on rank 0 at N = 1; kept for old command lines)')
    ap.add_argument('--no-inference', action='store_true', help='(--full) skip BASELINE config C5 (inf images/sec)')
    ap.add_argument('--no-fit-path', action='store_true', help='(--full) skip the reference main_train.py throughput leg (fit_path)')
    ap.add_argument('--no-c4', action='store_true', help='(--full) skip BASELINE config C4 (R-FCN head, 16 chips) at one GPU\'s share')
    ap.add_argument('--dump-outputs', metavar='DIR', help='write what the last timed step computed to DIR/<name>.npy (rank 0)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')

    # the host driver only supports dmabuf IPC: without this RCCL's peer mapping fails with hipIpcGetMemHandle: invalid argument
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit('launch with: python -m torch.distributed.run --nproc-per-node %d bench.py --gpus %d ...' %
                         (args.gpus, args.gpus))
    # one process per GPU; SNIPER_DIST_BACKEND=gloo + fewer devices than ranks is the single-GPU rehearsal of the N > 1
    # control flow (tests/test_gpu_engine.py), never a measurement
    torch.cuda.set_device(local % torch.cuda.device_count())
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group(backend=os.environ.get('SNIPER_DIST_BACKEND', 'nccl'))   # nccl = RCCL over xGMI

    from sniper_amd import hip
    from sniper_amd.train import Trainer
    tr = Trainer(batch_images=args.batch, n_images=48, seed=1000 * rank, rank_local=True)
    # a few distinct chip minibatches, resident in HBM before the timed region; their anchor-labelling inputs
    # (GT boxes per chip) are kept so that the labelling itself runs inside every step
    batches = [tr.batch] + [tr.next_batch() for _ in range(3)]
    import sniper_amd.mx as mx
    anchors = tr.iter.anchors

    packed = [anchors.pack_device(b.worker_data) for b in batches]     # GT boxes per chip: resident like the chips

    def step(i):
        b = batches[i % len(batches)]
        lab = anchors.assign(packed=packed[i % len(batches)], seed=i)
        label = [mx.nd.NDArray(lab['label']), mx.nd.NDArray(lab['bbox_target']), mx.nd.NDArray(lab['bbox_weight']),
                 mx.nd.NDArray(lab['gt_boxes'])]
        outs = tr.step(mx.io.DataBatch(data=b.data, label=label, pad=0, index=None, provide_data=b.provide_data,
                                       provide_label=b.provide_label))
        return lab, outs

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    for i in range(args.warmup):
        step(i)
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        last = step(i)
    host_dt = time.perf_counter() - t0     # host enqueue time: all launches issued, nothing waited for yet
    device = device_identity(local % torch.cuda.device_count())      # clocks sampled while the queued steps still run
    sync()
    dt = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([dt], device='cuda', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = dt / args.steps * 1e3
    value = world * args.batch * args.steps / dt
    ex = tr.mod.exe
    head = {
        'metric': 'train chips/sec (512x512, R101)', 'value': round(value, 2), 'unit': 'chips/s', 'n_gpus': world,
        'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': round(ms_per_step, 3), 'higher_is_better': True,
        'scaling': 'weak', 'vs_baseline': None, 'dtype': 'f16', 'data': 'synthetic',
        'host_enqueue_ms_per_step': round(host_dt / args.steps * 1e3, 3), 'graphs': bool(ex.use_graphs and ex._graph_fb is not None),
        'config': {'workload': 'ResNet-101 Faster-RCNN SNIPER 3-scale, batch %d x 512x512 fp16 per GPU (BASELINE configs[1]); '
                               'step = GPU anchor labelling + fwd + bwd + grad all-reduce + SGD on HBM-resident chips (epoch chip generation / box '
                               'assignment and image decode+resize are outside the step); f16 MFMA operands, f32 accumulation / losses / '
                               'master weights' % args.batch,
                   'chips_per_gpu': args.batch, 'global_batch': args.batch * world, 'parallelism': 'dp%d' % world},
        'device': dict(device, sampled='sysfs levels read after the timed steps were enqueued, before the closing synchronise '
                                       '(the device is still executing them)'),
    }
    if args.dump_outputs and rank == 0:
        # before any further step: the network outputs are the executor's buffers, which the next step overwrites
        head['dump_outputs'] = {'dir': args.dump_outputs, 'arrays': dump_outputs(args.dump_outputs, last[0], last[1],
                                                                                 tr.mod.output_names, tr.mod.get_params()[0])}
    if not args.full:
        # a plain run ends here: everything below runs steps, passes or processes of its own
        if rank == 0:
            print(json.dumps(head), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return

    # ---- host cost of one step with an idle device: enqueue only, nothing waited for (host_dt above is throttled by the
    # launch queue once the host runs ahead of the device, so it is an upper bound, not the host's own time)
    sync()
    t1 = time.perf_counter()
    step(0)
    host_idle_ms = (time.perf_counter() - t1) * 1e3
    sync()

    # ---- roofline of the dominant kernel family, live HIP-event timing (untimed extra steps)
    # The timed region replays hipGraphs; for per-launch HIP events the same step is run eagerly (same kernels, same
    # streams), bracketing every conv-family launch with events on the stream it is launched on.  EVERY rank runs these
    # extra steps: a step contains the gradient all-reduce, and a collective entered by rank 0 alone would never return.
    saved = (ex.use_graphs, ex._graph_fb, ex._graph_up)
    ex.use_graphs, ex._graph_fb, ex._graph_up = False, None, None
    def profile():
        step(0)                                     # settle (allocations of the eager path)
        with ConvProfiler() as prof:
            for i in range(2):
                step(i)
            res = prof.summary()
            profile.overhead_us = prof.overhead_ms * 1e3
            profile.by_shape = prof.shape_table(2)
            return res
    tot_ms, tot_fl, per = profile()                 # in situ: the kernels and the stream of the timed region, launched eagerly
    iso_ms, iso_fl, iso_per = tot_ms, tot_fl, per   # (one stream since round 3: a launch's duration is its own)
    ex.use_graphs, ex._graph_fb, ex._graph_up = saved
    achieved = tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0
    isolated = iso_fl / (iso_ms * 1e-3) / 1e12 if iso_ms > 0 else 0.0
    n_launch = sum(v[0] for v in per.values())
    roof = {'bound': 'mfma',
            'kernel': 'conv_dma_kernel<DGRAD,BM,BN,...> / wgrad_ps_kernel (+ conv_igemm_kernel for narrow layers, '
                      'wgrad_reduce_batch_kernel): sn_conv_fwd, sn_conv_fwd_stats, sn_conv_dgrad, sn_conv_dgrad_bn, sn_conv_wgrad_batch',
            'achieved': round(achieved, 2), 'peak': MFMA_PEAK_TFLOPS, 'unit': 'TFLOP/s', 'frac': round(achieved / MFMA_PEAK_TFLOPS, 4),
            'mode': 'in situ (eager replay of the timed step on its one stream); sum of launch durations as rocprofv3 --kernel-trace '
                    '--stats reports them',
            'achieved_isolated': round(isolated, 2), 'frac_isolated': round(isolated / MFMA_PEAK_TFLOPS, 4),
            'step_tflops': round(tot_fl / 2 / (ms_per_step * 1e-3) / 1e12, 2), 'event_bracket_overhead_us': round(profile.overhead_us, 2),
            'traffic': pmc_traffic(),         # HBM bytes per KERNEL launch of the family (incl. the slab-reduce kernels)
            'traffic_detail': getattr(pmc_traffic, 'detail', None),
            'roofline_hbm': roofline_hbm(),      # the memory-bound kernels of the step (RoI pooling, sampling, BatchNorm, NMS, labelling)
            'entry_calls_per_step': n_launch // 2,   # C-ABI calls bracketed with events (one batched weight-gradient call = up to 24 layers)
            'avg_launch_ms': round(tot_ms / max(1, n_launch), 4),
            'gflop_per_step': round(tot_fl / 2 / 1e9, 1), 'conv_ms_per_step': round(tot_ms / 2, 3),
            'conv_ms_per_step_isolated': round(iso_ms / 2, 3),
            'by_shape': profile.by_shape,
            'by_entry': {k: {'launches': v[0] // 2, 'ms_per_step': round(v[1] / 2, 3),
                             'tflops': round(v[2] / (v[1] * 1e-3) / 1e12, 1) if v[1] > 0 else 0.0} for k, v in per.items()}}
    dist_report = None
    if dist is not None:
        dist_report = dist_probe(tr, step, sync, dist, world)
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        try:
            cpu = cpu_baseline()
        except Exception as e:   # the baseline is a report, never a reason to lose the measurement
            cpu = {'value': None, 'unit': 'chips/s', 'cores': os.cpu_count(), 'kind': 'port', 'sample': 'failed: %r' % (e,)}
        try:
            cpu['c1'] = cpu_c1_step()
        except Exception as e:   # noqa: BLE001
            cpu['c1'] = {'value': None, 'sample': 'failed: %r' % (e,)}
        # the SAME epoch chip database built through the reference's unchanged MNIteratorE2E.reset over the extension mirrors
        # (its Pool = the drop-in pool that batches chip_worker maps into ragged GPU launches): tools/chipdb_bench.py, own process
        try:
            import subprocess
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'chipdb_bench.py'), '5000', '400'], cwd=ROOT,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600,
                               env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
            cpu['chip_db_through_shim'] = json.loads(lines[-1]) if r.returncode == 0 and lines else \
                {'value': None, 'sample': 'failed (rc %d): %s' % (r.returncode, r.stderr[-400:])}
        except Exception as e:   # noqa: BLE001
            cpu['chip_db_through_shim'] = {'value': None, 'sample': 'failed: %r' % (e,)}
    fit_path = None
    if rank == 0 and world == 1 and not args.no_fit_path:
        # what a user of the drop-in gets: the reference's unchanged main_train.py -- PrefetchingIter + mod.fit +
        # its six EvalMetrics + Speedometer -- at BATCH_IMAGES 20 over the lib/iterators mirrors, images decoded from JPEG files,
        # chips/s from wall time over 50 batches; own process, on this card right after the timed steps (tools/fit_path_bench.py)
        try:
            import subprocess
            torch.cuda.empty_cache()
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'fit_path_bench.py'), 'mirror', str(args.batch), '50'], cwd=ROOT,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=420,
                               env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
            fit_path = json.loads(lines[-1]) if lines else {'value': None, 'sample': 'failed (rc %d): %s' % (r.returncode, r.stderr[-400:])}
            if fit_path.get('value'):
                fit_path['ratio_to_value'] = round(fit_path['value'] / value, 3)
            # the same main_train.py with the reference's OWN lib/iterators + lib/data_utils on the drop-in pool (per-batch worker maps
            # routed to batched GPU work, batches born in HBM through the shim's unplaced mx.nd.zeros)
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'fit_path_bench.py'), 'reference', str(args.batch), '40'], cwd=ROOT,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=420,
                               env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
            ref_it = json.loads(lines[-1]) if lines else {'value': None, 'sample': 'failed (rc %d): %s' % (r.returncode, r.stderr[-400:])}
            fit_path['reference_iterator'] = ref_it
            if ref_it.get('value'):
                fit_path['reference_iterator_value'] = ref_it['value']
                fit_path['reference_iterator_ratio'] = round(ref_it['value'] / value, 3)
        except Exception as e:   # noqa: BLE001 -- a report
            fit_path = {'value': None, 'sample': 'failed: %r' % (e,)}
    c4 = None
    if rank == 0 and world == 1 and not args.no_c4:
        # BASELINE configs[3] (R-FCN / PS-RoI pooling head) at one GPU's share -- 16 chips -- in its own process (tools/c4_bench.py):
        # chips/s, ms per step, the head's own ms; HBM rows of the three position-sensitive kernels from the counter passes
        try:
            import subprocess
            torch.cuda.empty_cache()
            r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'c4_bench.py'), '20', '5', '16'], cwd=ROOT, stdout=subprocess.PIPE,
                               stderr=subprocess.PIPE, text=True, timeout=420, env=dict(os.environ, PYTHONDONTWRITEBYTECODE='1'))
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
            c4 = json.loads(lines[-1]) if lines else {'value': None, 'sample': 'failed (rc %d): %s' % (r.returncode, r.stderr[-400:])}
            c4['roofline_hbm'] = roofline_hbm('pmc_c4_kernels.json', C4_HBM_KERNELS)
        except Exception as e:   # noqa: BLE001 -- a report
            c4 = {'value': None, 'sample': 'failed: %r' % (e,)}
    if rank == 0:
        out = dict(head, host_enqueue_idle_device_ms=round(host_idle_ms, 3),
                   rpn_heads_dtype='f16 MFMA operands, f32 accumulate (reference: f32 after its Cast, resnet_mx_101_e2e.py:250-252)',
                   library_sources_hash=library_sources_hash(), roofline=roof, cpu_baseline=cpu)
        if dist_report is not None:
            out['dist'] = dist_report
        if fit_path is not None:
            out['fit_path'] = fit_path
        if c4 is not None:
            out['c4'] = c4
        # the committed rocprofv3 --kernel-trace --stats cross-check of this same command ON THIS BUILD (tools/roofline_check.py,
        # same session as a bench line of that card): lets a reader tell card-to-card spread from a regression
        try:
            with open(os.path.join(ROOT, 'profiles', 'roofline_check.json')) as fh:
                rc = json.load(fh)
            if rc.get('library_sources_hash') == out['library_sources_hash']:
                roof['rocprof_cross_check'] = {k: rc.get(k) for k in ('frac_rocprof', 'tflops_rocprof', 'bench_frac', 'ratio_bench_over_rocprof',
                                                                       'conv_family_ms_per_step_rocprof', 'device')}
        except (OSError, ValueError):
            pass
        if not args.no_inference and world == 1:
            out['inference'] = bench_inference()
        # the full record (per-shape tables, per-kernel HBM rows, sample prose) goes to a file and to a line printed BEFORE the final
        # one; the final line is the compact record a log tail of a few KB still holds whole (tests/test_bench_line.py)
        detail = json.dumps(out)
        for d in ('gpurun_out', 'profiles'):
            try:
                os.makedirs(os.path.join(ROOT, d), exist_ok=True)
                with open(os.path.join(ROOT, d, 'bench_detail.json'), 'w') as fh:
                    fh.write(detail + '\n')
                break
            except OSError:
                continue
        print('BENCH_DETAIL ' + detail, flush=True)
        print(json.dumps(compact_line(out)), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
