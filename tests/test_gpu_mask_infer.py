"""GPU: the mask head at test time -- sn_mask_class_prob against its float64 reference within the derived
bound (tests/mask_infer_util.py), an exact-arithmetic case, the fused graph against the stock chain on the engine and against
oracle/graph_cpu.py, MaskTester end to end with a head whose answer is known, and the reuse of bound shapes."""
import numpy as np
import pytest
import torch

from gpu_util import assert_close, dev, f16r
from mask_infer_util import EDGE_CLASSES, U, edge_classes, mask_class_prob_bound, mask_class_prob_ref, mask_logits_ref, softmax1

pytestmark = pytest.mark.gpu

CANARY, PAD = 7.0, 64


def _hip():
    from sniper_amd import hip
    hip.require_gpu()
    return hip


def _run_kernel(hip, x16, w16, bias, cls, K):
    """-> prob (N, HW) float32 numpy; the canaries around the output must be untouched, and a second launch gives the same bits"""
    N, HW, C = x16.shape
    xd, wd = torch.from_numpy(x16).to(dev()), torch.from_numpy(w16).to(dev())
    bd = None if bias is None else torch.from_numpy(bias).to(dev())
    cd = torch.from_numpy(cls).to(dev())
    outs = []
    for _ in range(2):
        buf = torch.full((N * HW + 2 * PAD,), CANARY, dtype=torch.float32, device=dev())
        hip.call('sn_mask_class_prob', xd, wd, bd, cd, buf[PAD:], N, HW, C, K, hip.stream())
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:PAD] == CANARY).all() and (h[PAD + N * HW:] == CANARY).all(), 'the kernel wrote outside prob'
        outs.append(h[PAD:PAD + N * HW].reshape(N, HW).copy())
    assert np.array_equal(outs[0], outs[1]), 'two launches on the same inputs differ'
    return outs[0]


# (N, HW, C, K): one pixel; a pixel count that fills neither a wave's tile nor a workgroup; a channel count that is no multiple of the
# 256-channel pass (one full pass + 8); the real shape (784 = 12 workgroups + a 16-pixel rest); more RoIs than the other cases with a
# pixel count below one workgroup
SHAPES = [(1, 1, 8, 1), (3, 9, 24, 2), (2, 65, 264, 80), (5, 784, 256, 80), (301, 49, 256, 80)]


@pytest.mark.parametrize('with_bias', [False, True], ids=['nobias', 'bias'])
@pytest.mark.parametrize('shape', SHAPES, ids=['x'.join(map(str, s)) for s in SHAPES])
def test_kernel_against_reference_within_the_derived_bound(shape, with_bias):
    hip = _hip()
    N, HW, C, K = shape
    rs = np.random.RandomState(N * 1000 + HW)
    x16 = np.maximum(rs.standard_normal((N, HW, C)), -0.3).astype(np.float16)             # ReLU-like: many equal values, some negative
    w16 = (rs.standard_normal((2 * K, C)) * (2.0 / np.sqrt(C))).astype(np.float16)
    bias = (rs.standard_normal(2 * K) * 0.7).astype(np.float32) if with_bias else None
    seen = set()
    for start in range(0, EDGE_CLASSES, N):                  # (N < 5: several launches, until every out-of-range class was used)
        cls = edge_classes(N, K, rs, start)
        seen |= set(cls[:2 * EDGE_CLASSES].astype(int).tolist())
        got = _run_kernel(hip, x16, w16, bias, cls, K)
        want = mask_class_prob_ref(x16, w16, bias, cls, K)
        bound = mask_class_prob_bound(x16, w16, bias, cls, K)
        err = np.abs(got.astype(np.float64) - want)
        print('shape %s bias %s start %d: max err %.3e, max err / bound %.3f, bound <= %.3e' % (shape, with_bias, start, err.max(),
                                                                                          (err / bound).max(), bound.max()))
        assert np.isfinite(got).all()
        assert (err <= bound).all(), (shape, start, float(err.max()), float((err / bound).max()))
        assert want.max() - want.min() > 0.3 or N * HW < 4       # not a constant output
    assert {0, K - 1, -1, K, 2 * K + 5} <= seen


def test_exact_arithmetic_case():
    """Small integers times powers of two, biases of 2048 + an integer: every partial sum of a logit is exact in float32 in ANY
    order, so the kernel's logits ARE the reference's and its output must be, bit for bit, what sn_softmax_fwd makes of the exact
    logits (a logit rounded to fp16 on the way -- spacing 2 at 2048 -- would not survive this).  Equal logits give exactly 0.5."""
    hip = _hip()
    N, HW, C, K = 7, 45, 264, 3
    rs = np.random.RandomState(11)
    x = rs.randint(0, 3, (N, HW, C)).astype(np.float16)
    w = np.zeros((2 * K, C), np.float16)
    for r in range(2 * K):
        at = rs.choice(C, 6, replace=False)
        at[0], at[1] = 256 + (r % 8), 255 - r                     # both passes, the last lane of the first and the only lane of the second
        w[r, at] = rs.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], 6)
    bias = (2048 + rs.randint(-3, 4, 2 * K)).astype(np.float32)
    cls = np.array([0, 1, 2, -1, K, 2 * K + 5, 1], np.float32)        # 2K + 5: neg = pos = 2K - 1, equal logits
    zn, zp, an, ap = mask_logits_ref(x, w, bias, cls, K)
    assert max(an.max(), ap.max()) < 2 ** 13 and np.array_equal(zn * 2, np.round(zn * 2))      # exact in float32: < 2^13 in steps of 1/2
    got = _run_kernel(hip, x, w, bias, cls, K)
    logits = torch.from_numpy(np.stack([zn, zp], 1).astype(np.float32)).to(dev())                  # (N, 2, HW), exact
    p = torch.empty_like(logits)
    hip.call('sn_softmax_fwd', logits, p, N, 2, HW, hip.stream())
    torch.cuda.synchronize()
    want = p[:, 1].cpu().numpy()
    assert np.array_equal(got, want), np.abs(got.astype(np.float64) - want).max()
    assert (got[5] == 0.5).all() and np.array_equal(zn[5], zp[5])
    assert np.abs(got - softmax1(zn, zp)).max() <= 8 * U
    d = np.abs(zn - zp)
    assert ((d > 0) & (d < 8)).mean() > 0.3                      # most outputs are not saturated: a wrong logit shows


# ---- the lowering: fused graph against the stock chain -------------------------------------------------------------------------
def _step_values(ex):
    """{node name: the step's output in reference order} as tests/test_gpu_engine.py::_forced_parity collects them (an output that holds
    a fused successor's values is left to that successor's node)"""
    vals = {}
    for st in ex.steps:
        y = getattr(st, 'y', None)
        kind = type(st).__name__
        if y is None or y.t is None or (kind == 'BatchNormStep' and getattr(st, 'act', 0)) or \
                getattr(st, 'fused_residual', None) is not None or getattr(st, 'fold_bn', None) is not None or \
                (kind == 'BatchNormStep' and getattr(st, 'folded_into', None) is not None and not getattr(st, 'act', 0)):
            continue
        t = y.t.float()
        if y.fmt == 'act' and len(y.shape) == 4:
            t = t.permute(0, 3, 1, 2)
        if int(np.prod(y.shape)) != t.numel():
            continue
        vals[st.node.name] = t.reshape(y.shape).cpu().numpy()
    return vals


def test_fused_graph_against_the_stock_chain_and_the_cpu_oracle():
    import os
    from test_gpu_engine import _init_params
    from oracle import graph_cpu
    from sniper_amd import config as cfgmod
    from sniper_amd.engine.executor import Executor
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    _hip()
    K, R = 80, 8
    cfg = cfgmod.res101_e2e_mask(batch_images=1)
    shapes = dict(data=(1, 3, 128, 160), mask_rois=(R, 5), mask_cls=(R,))
    syms = {f: mk.resnet_mx_101_e2e_mask(test_nbatch=1).get_symbol_mask_test(cfg, R, fused=f) for f in (True, False)}
    rs = np.random.RandomState(23)
    P, AUX = _init_params(syms[False], shapes, rs, bn_gamma=(0.5, 1.0), bn_beta=(-0.2, 0.4))
    for k in P:
        if k.startswith('mask_') and k.endswith('_weight') and 'offset' not in k:
            P[k] = f16r(rs.standard_normal(P[k].shape) * np.sqrt(2.0 / np.prod(P[k].shape[1:])))
    # (the random head's activations reach the hundreds: a small mask_out keeps the logits in the range where the softmax resolves them)
    P['mask_out_weight'] = f16r(P['mask_out_weight'] * 0.01)
    P['mask_out_bias'] = (rs.standard_normal(2 * K) * 0.5).astype(np.float32)
    P['bn_data_gamma'][:] = 1.0
    AUX['bn_data_moving_mean'][:] = 0.0
    AUX['bn_data_moving_var'][:] = 1.0 - 2e-5
    P['bn_data_beta'][:] = 0.0
    rois = np.array([[0, 10, 12, 90, 70], [0, 30, 20, 110, 100],          # two overlapping
                     [0, 100, 60, 159, 127], [0, 0, 0, 40, 127],           # at the image border
                     [0, 64, 40, 72, 50], [0, 5, 90, 150, 120], [0, 50, 50, 50, 50],
                     [0, 0, 0, 0, 0]], np.float32)                         # the padding row
    cls = np.array([3, 79, 0, 41, 17, 78, 5, 0], np.float32)
    inp = dict(data=f16r(rs.standard_normal((1, 3, 128, 160)) * 50), mask_rois=rois, mask_cls=cls)
    os.environ['SNIPER_HIP_GRAPHS'] = '0'
    try:
        exs = {f: Executor(syms[f], shapes, False) for f in (True, False)}
    finally:
        os.environ.pop('SNIPER_HIP_GRAPHS', None)
    out, xs = {}, {}
    for f, ex in exs.items():
        ex.set_params(P, AUX)
        o = ex.forward(inp, is_train=False)
        torch.cuda.synchronize()
        out[f] = mk.resnet_mx_101_e2e_mask.mask_prob_of(o[0].cpu().numpy())
        head = [st for st in ex.steps if st.node.name in ('mask_prob', 'mask_out')][0]
        xs[f] = head.x.t.cpu().numpy().astype(np.float32).reshape(R, 28 * 28, 256)                 # mask_deconv_relu, channels-last
    assert out[True].shape == out[False].shape == (R, 28, 28)
    assert np.array_equal(xs[True], xs[False]), 'the two graphs are the same network up to mask_deconv_relu'
    assert (xs[True] > 0).mean() > 0.05
    # (1) the fused operator on the device's own head input, with the weights in the CHECKPOINT's layout: lowering + weight layout
    w = f16r(P['mask_out_weight']).reshape(2 * K, 256)
    want = mask_class_prob_ref(xs[True], w, P['mask_out_bias'], cls, K).reshape(R, 28, 28)
    bound = mask_class_prob_bound(xs[True], w, P['mask_out_bias'], cls, K).reshape(R, 28, 28)
    err = np.abs(out[True] - want)
    print('fused vs reference: max err %.3e, max err / bound %.3f' % (err.max(), (err / bound).max()))
    assert (err <= bound).all(), float((err / bound).max())
    # (2) fused against the stock chain: they differ by the fp16 rounding of the stock chain's logits, 2^-11 relative each
    zn, zp, _, _ = mask_logits_ref(xs[True], w, P['mask_out_bias'], cls, K)
    tol = (0.25 * 2.0 ** -11 * (np.abs(zn) + np.abs(zp))).reshape(R, 28, 28) + bound
    diff = np.abs(out[True].astype(np.float64) - out[False])
    print('fused vs stock chain: max diff %.3e, max diff / tolerance %.3f; logits up to %.2f' % (diff.max(), (diff / tol).max(),
                                                                                           max(np.abs(zn).max(), np.abs(zp).max())))
    assert (diff <= tol).all(), float((diff / tol).max())
    assert np.abs(zn - zp).max() > 0.5 and out[True].std() > 0.02             # the head's answer varies over the RoIs
    # (3) the stock-chain graph, trunk to mask, on oracle/graph_cpu.py, teacher-forced like test_r101_mask_network_parity_vs_cpu_reference_ops
    dev_vals = _step_values(exs[False])
    want_cpu, _ = graph_cpu.run(syms[False], P, AUX, inp, is_train=False, want_grads=False, fp16_storage=True, force=dev_vals)
    le = graph_cpu.run.local_err
    assert len(le) > 0.8 * len(dev_vals) and 'mask_out' in le and 'mask_deconv_relu' in le
    worst = max(le, key=le.get)
    assert le[worst] <= 1e-2, 'forward mismatch %.5f at node %s' % (le[worst], worst)
    cpu = mk.resnet_mx_101_e2e_mask.mask_prob_of(np.asarray(want_cpu[0]))
    zmax = float(max(np.abs(zn).max(), np.abs(zp).max()))
    for f in (True, False):
        assert_close(out[f], cpu, 0.0, 0.25 * 2 * 1e-2 * zmax + 1e-5, 'mask_prob vs the CPU oracle (fused=%s)' % f)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _random_params(sym, shapes, rs):
    from test_gpu_engine import _init_params
    P, AUX = _init_params(sym, shapes, rs, bn_gamma=(0.5, 1.0), bn_beta=(-0.2, 0.4))
    return P, AUX


def _rect_rle(box, h, w):
    m = np.zeros((h, w), np.uint8)
    m[box[1]:box[3] + 1, box[0]:box[2] + 1] = 1
    flat = m.T.reshape(-1)                                        # column-major
    edges = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], edges, [flat.size]]))
    if flat[0] == 1:
        runs = np.concatenate([[0], runs])
    return {'size': [h, w], 'counts': runs.astype(np.int64)}


def test_predict_masks_end_to_end_with_a_known_head():
    from sniper_amd import config as cfgmod
    from sniper_amd.evaluation import evaluate_sds, paste_boxes
    from sniper_amd.mask_inference import predict_masks
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    from sniper_amd.synthetic import make_roidb
    _hip()
    K, NC, R = 80, 81, 6
    cfg = cfgmod.res101_e2e_mask(batch_images=1)
    rs = np.random.RandomState(31)
    roidb = make_roidb(3, seed=5, with_masks=True)
    for r in roidb:
        r['image'] = rs.randint(0, 256, (r['height'], r['width'], 3)).astype(np.uint8)
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in roidb] for _ in range(NC)]
    for i, r in enumerate(roidb):
        for c in np.unique(r['gt_classes']):
            rows = r['boxes'][r['gt_classes'] == c]
            all_boxes[int(c)][i] = np.concatenate([rows, rs.uniform(0.3, 1.0, (len(rows), 1))], 1).astype(np.float32)
    all_boxes[0] = [np.zeros((0, 5), np.float32) for _ in roidb]
    per_image = [sum(len(all_boxes[c][i]) for c in range(1, NC)) for i in range(len(roidb))]
    assert max(per_image) > R, 'one image must need a second pass'
    sym = mk.resnet_mx_101_e2e_mask().get_symbol_mask_test(cfg, R)
    P, AUX = _random_params(sym, dict(data=(1, 3, 128, 192), mask_rois=(R, 5), mask_cls=(R,)), rs)
    P['mask_out_weight'][:] = 0.0
    b = np.zeros(2 * K, np.float32)
    odd = np.arange(K) % 2 == 1
    b[:K] = np.where(odd, -8.0, 8.0)
    b[K:] = np.where(odd, 8.0, -8.0)
    P['mask_out_bias'] = b
    all_masks = predict_masks(mk.resnet_mx_101_e2e_mask, cfg, roidb, all_boxes, P, AUX, scale=(128, 192), rois_per_image=R)
    assert len(all_masks) == NC and all(len(m) == len(roidb) for m in all_masks)
    want_masks = [[[] for _ in roidb] for _ in range(NC)]
    n_odd = n_even = 0
    for c in range(NC):
        for i, r in enumerate(roidb):
            cell = all_masks[c][i]
            assert cell.shape == (len(all_boxes[c][i]), 28, 28) and cell.dtype == np.float32, (c, i, cell.shape)
            if not len(cell):
                continue
            if (c - 1) % 2 == 1:
                assert cell.min() > 0.99, (c, i, float(cell.min()))
                n_odd += len(cell)
                want_masks[c][i] = [_rect_rle(bx, r['height'], r['width']) for bx in paste_boxes(all_boxes[c][i], r['height'], r['width'])]
            else:
                assert cell.max() < 0.01, (c, i, float(cell.max()))
                n_even += len(cell)
                want_masks[c][i] = [{'size': [r['height'], r['width']], 'counts': np.array([r['height'] * r['width']], np.int64)}
                                    for _ in range(len(cell))]
    assert n_odd >= 3 and n_even >= 3 and len(all_masks[0][0]) == 0
    got = evaluate_sds(all_boxes, all_masks, roidb, NC)
    want = evaluate_sds(all_boxes, want_masks, roidb, NC)
    assert np.array_equal(got.precision, want.precision) and np.array_equal(got.recall, want.recall)
    assert (want.precision > -1).any() and (want.recall > -1).any()          # some (category, area range) was evaluated at all


def test_two_images_of_one_bucket_share_an_executor():
    from sniper_amd import config as cfgmod
    from sniper_amd.mask_inference import MaskTester
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    _hip()
    cfg = cfgmod.res101_e2e_mask(batch_images=1)
    rs = np.random.RandomState(2)
    sizes = [(100, 150), (110, 140), (150, 100)]                  # (h, w): 128 x 192 and 128 x 163 share the bucket (128, 192); portrait
    roidb = [dict(image=rs.randint(0, 256, (h, w, 3)).astype(np.uint8), height=h, width=w, flipped=False) for h, w in sizes]
    NC, R = 81, 4
    one = lambda i: [[(np.array([[5, 5, 60, 70, 0.9]], np.float32) if (c == 7 and j == i) else np.zeros((0, 5), np.float32))
                      for j in range(3)] for c in range(NC)]
    tester = MaskTester(mk.resnet_mx_101_e2e_mask(), cfg, None, None, scale=(128, 192), rois_per_image=R)
    assert tester.bound_executors() == 0
    m0 = tester.predict(roidb, one(0))
    assert tester.bound_executors() == 1 and tester.passes == 1
    m1 = tester.predict(roidb, one(1))
    assert tester.bound_executors() == 1 and tester.passes == 1, 'an image of the same 64-pixel bucket must reuse the executor'
    m2 = tester.predict(roidb, one(2))
    assert tester.bound_executors() == 2 and tester.passes == 1
    for i, m in enumerate((m0, m1, m2)):
        assert m[7][i].shape == (1, 28, 28) and np.isfinite(m[7][i]).all() and 0 <= m[7][i].min() <= m[7][i].max() <= 1
        assert sum(len(m[c][j]) for c in range(NC) for j in range(3)) == 1
    none = [[np.zeros((0, 5), np.float32) for _ in range(3)] for _ in range(NC)]
    tester.predict(roidb, none)
    assert tester.passes == 0                                      # no detections: no pass
