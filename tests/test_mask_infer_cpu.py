"""CPU: the mask head at test time -- the test graph's parameters and shapes, the stock output chain on
oracle/graph_cpu.py against the float64 reference of sn_mask_class_prob (so the header's clipping rule IS the stock chain's), the
entry point's refusals, the kernel's register budget and the row bookkeeping of MaskTester.  Nothing here needs a device."""
import ctypes
import os

import numpy as np
import pytest

from mask_infer_util import EDGE_CLASSES, class_rows, edge_classes, mask_class_prob_bound, mask_class_prob_ref

K = 80


def _cfg():
    from sniper_amd import config as cfgmod
    return cfgmod.res101_e2e_mask(batch_images=2)


def _mk():
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    return mk


# ---- graph -----------------------------------------------------------------------------------------------------------------
def test_mask_test_graph_parameters_are_the_training_graphs():
    mk, cfg = _mk(), _cfg()
    A, F, B, R = 21, 32, 2, 7
    train = mk.resnet_mx_101_e2e_mask().get_symbol_rcnn(cfg)
    tshapes = dict(data=(2, 3, 512, 512), valid_ranges=(2, 2), im_info=(2, 3), label=(2, A * F * F), bbox_target=(2, 4 * A, F, F),
                   bbox_weight=(2, 4 * A, F, F), gt_boxes=(2, 100, 5), gt_masks=(2, 100, 500))
    targs, _, tauxs = train.infer_shape(**tshapes)
    tdict = dict(zip(train.list_arguments(), targs))
    tdict.update(zip(train.list_auxiliary_states(), tauxs))
    inputs = {'data', 'mask_rois', 'mask_cls'}
    params = {}
    for fused in (True, False):
        sym = mk.resnet_mx_101_e2e_mask(test_nbatch=B).get_symbol_mask_test(cfg, R, fused=fused)
        assert inputs <= set(sym.list_arguments())
        args, outs, auxs = sym.infer_shape(data=(B, 3, 128, 192), mask_rois=(B * R, 5), mask_cls=(B * R,))
        got = dict(zip(sym.list_arguments(), args))
        got.update(zip(sym.list_auxiliary_states(), auxs))
        params[fused] = {k: v for k, v in got.items() if k not in inputs}
        assert set(params[fused]) <= set(tdict), sorted(set(params[fused]) - set(tdict))
        assert all(tdict[k] == v for k, v in params[fused].items())
        assert outs == [(B * R, 1 if fused else 2, 28, 28)]
    assert params[True] == params[False]
    for name in ('mask_out_weight', 'mask_out_bias', 'mask_deconv_weight', 'mask_conv_3x3_4_weight', 'mask_offset_weight', 'conv_new_1_weight'):
        assert name in params[True]
    assert params[True]['mask_out_weight'] == (2 * K, 256, 1, 1) and params[True]['mask_out_bias'] == (2 * K,)
    assert not any(k.startswith(('rpn_', 'fc_new', 'cls_score', 'bbox_pred')) for k in params[True])
    sym = mk.resnet_mx_101_e2e_mask().get_symbol_mask_test(cfg)
    assert sym.list_outputs() == ['mask_prob_output']


def test_mask_test_graph_lowers_without_a_device():
    """fused: ONE MaskClassProb step holding mask_out's parameters like a 1x1 convolution's, no mask_out convolution, pick, Concat or
    softmax; stock chain: exactly those.  An executor built for training refuses the operator by the node's name."""
    import torch
    from sniper_amd.engine.executor import Executor
    mk, cfg = _mk(), _cfg()
    B, R = 1, 5
    shapes = dict(data=(B, 3, 128, 192), mask_rois=(B * R, 5), mask_cls=(B * R,))
    kinds = {}
    for fused in (True, False):
        sym = mk.resnet_mx_101_e2e_mask(test_nbatch=B).get_symbol_mask_test(cfg, R, fused=fused)
        ex = Executor(sym, shapes, False, device=torch.device('cpu'))
        kinds[fused] = [type(s).__name__ for s in ex.steps]
        w, b = ex.params['mask_out_weight'], ex.params['mask_out_bias']
        assert (w.kind, tuple(w.int_shape), tuple(w.ref_shape)) == ('conv', (2 * K, 1, 256), (2 * K, 256, 1, 1)) and tuple(b.int_shape) == (2 * K,)
        assert not w.trainable and not b.trainable
        head = ex.steps[-1]
        if fused:
            assert type(head).__name__ == 'MaskClassProbStep' and head.K == K and head.y.fmt == 'f32' and head.y.shape == (B * R, 1, 28, 28)
            assert head.x.fmt == 'act' and head.x.shape == (B * R, 256, 28, 28) and head.x.producer.node.name == 'mask_deconv_relu'
            assert head.w is w and head.b is b
        else:
            assert type(head).__name__ == 'SoftmaxActivationStep' and head.y.shape == (B * R, 2, 28, 28)
    tail = ('PickStep', 'SoftmaxActivationStep')            # (the trunk's cat4 is a Concat in both graphs)
    assert kinds[True].count('MaskClassProbStep') == 1 and not any(k in tail for k in kinds[True])
    assert kinds[False].count('PickStep') == 2 and kinds[False].count('ConcatStep') == kinds[True].count('ConcatStep') + 1
    assert 'MaskClassProbStep' not in kinds[False]
    assert kinds[False].count('ConvolutionStep') == kinds[True].count('ConvolutionStep') + 1
    sym = mk.resnet_mx_101_e2e_mask(test_nbatch=B).get_symbol_mask_test(cfg, R, fused=True)
    with pytest.raises(NotImplementedError) as e:
        Executor(sym, shapes, True, device=torch.device('cpu'))
    assert 'mask_prob' in str(e.value) and 'test-time' in str(e.value)


# ---- the stock chain on the CPU oracle = the reference of the fused kernel ------------------------------------------------------
def test_stock_output_chain_on_the_oracle_equals_the_reference():
    import sniper_amd.mx as mx
    from oracle import graph_cpu
    mk = _mk()
    rs = np.random.RandomState(3)
    N, C, S = 2 * EDGE_CLASSES, 256, 28
    x = np.maximum(rs.standard_normal((N, C, S, S)), 0).astype(np.float16).astype(np.float32)
    w = (rs.standard_normal((2 * K, C, 1, 1)) * 0.05).astype(np.float16).astype(np.float32)
    b = (rs.standard_normal(2 * K) * 0.5).astype(np.float32)
    cls = edge_classes(N, K, rs)
    assert {0, K - 1, -1, K, 2 * K + 5} <= set(cls.astype(int).tolist())
    sym = mk.resnet_mx_101_e2e_mask().get_mask_output(mx.sym.Variable(name='x'), mx.sym.Variable(name='mask_cls'), fused=False)
    outs, _ = graph_cpu.run(sym, {'mask_out_weight': w, 'mask_out_bias': b}, {}, {'x': x, 'mask_cls': cls}, is_train=False,
                            want_grads=False)
    got = mk.resnet_mx_101_e2e_mask.mask_prob_of(np.asarray(outs[0].detach().numpy() if hasattr(outs[0], 'detach') else outs[0]))
    x_nhwc = x.transpose(0, 2, 3, 1).reshape(N, S * S, C)
    want = mask_class_prob_ref(x_nhwc, w.reshape(2 * K, C), b, cls, K).reshape(N, S, S)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    assert want.min() < 0.2 and want.max() > 0.8                      # the comparison sees both ends of the range
    neg, pos = class_rows(cls, K)
    assert neg.tolist()[:5] == [0, K - 1, 0, K, 2 * K - 1] and pos.tolist()[:5] == [K, 2 * K - 1, K - 1, 2 * K - 1, 2 * K - 1]
    # the bound the GPU tests use is a bound: float32 arithmetic of the same sums in another order stays inside it
    z32 = lambda rows: np.einsum('npc,nc->np', x_nhwc.astype(np.float32), w.reshape(2 * K, C)[rows].astype(np.float32)) + b[rows][:, None]
    m = np.maximum(z32(neg), z32(pos))
    p32 = np.exp(z32(pos) - m) / (np.exp(z32(neg) - m) + np.exp(z32(pos) - m))
    assert (np.abs(p32.reshape(N, S, S) - want) <= mask_class_prob_bound(x_nhwc, w.reshape(2 * K, C), b, cls, K).reshape(N, S, S)).all()


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


P = ctypes.c_void_p(4096)


def _call(N=4, HW=784, C=256, K_=80, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_mask_class_prob', g('x'), g('w16'), g('bias'), g('cls'), g('prob'), N, HW, C, K_, None)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert (call[0] + ':') in msg and all(w in msg for w in words), msg


def test_every_refusal_comes_before_a_launch(lib):
    """(there is no device here and the pointers are not memory: a launch, or a dereference, would fail with another message)"""
    for name in ('x', 'w16', 'cls', 'prob'):
        _refused(lib, ('null pointer',), _call(**{name: None}))
    for kw in (dict(N=0), dict(HW=0), dict(C=0), dict(K_=0), dict(N=-3)):
        _refused(lib, ('at least 1',), _call(**kw))
    _refused(lib, ('C = 252', 'multiple of 8'), _call(C=252))
    _refused(lib, ('C = 4', 'multiple of 8'), _call(C=4))
    _refused(lib, ('32-bit indexing', '2147483648'), _call(N=1 << 13, HW=1 << 10, C=256))
    _refused(lib, ('32-bit indexing',), _call(N=1 << 20, HW=1 << 20, C=8))
    _refused(lib, ('16-byte aligned',), _call(x=ctypes.c_void_p(4096 + 8)))
    _refused(lib, ('16-byte aligned',), _call(w16=ctypes.c_void_p(4096 + 2)))


def test_symbol_is_exported_and_documented(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert 'sn_mask_class_prob' in {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    ret, argtypes, names = lib.protos['sn_mask_class_prob']
    assert names == ['x', 'w16', 'bias', 'cls', 'prob', 'N', 'HW', 'C', 'K', 'stream'] and ret is ctypes.c_int
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for doc in ('INTEGRATION.md', 'DESIGN.md', 'include/sniper_hip.h'):
        with open(os.path.join(root, doc)) as fh:
            assert 'sn_mask_class_prob' in fh.read(), doc
    with open(os.path.join(root, 'INTEGRATION.md')) as fh:
        text = fh.read()
    assert 'predict_masks' in text and 'MaskTester' in text


# ---- kernel resources ------------------------------------------------------------------------------------------------------------
def test_mask_class_prob_kernel_resources(lib):
    """One kernel; nothing in scratch, nothing spilled.  The workgroup is 256 threads = 4 waves, one per SIMD, and the kernel is built
    for at least 4 waves per SIMD (<= 128 VGPRs): 4 workgroups = 16 waves = 256 pixels' loads of 16 KB each in flight per CU."""
    from test_kernel_resources import _resources
    res = {k: v for k, v in _resources('mask_infer').items() if 'mask_class_prob_kernel' in k}
    assert len(res) == 1, sorted(res)
    (name, r), = res.items()
    assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
    assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4, (name, r)
    assert r.get('LDS Size', 0) == 0, (name, r)


# ---- row bookkeeping -------------------------------------------------------------------------------------------------------------
def _synthetic_boxes(rs, num_classes, n_images, R):
    """empty cells, an image with no detections (1), an image with R + 1 rows (2), one detection in the last class (3)"""
    all_boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(num_classes)]

    def rows(n):
        xy = rs.uniform(0, 300, (n, 2))
        return np.concatenate([xy, xy + rs.uniform(1, 200, (n, 2)), rs.uniform(0, 1, (n, 1))], 1).astype(np.float32)
    all_boxes[1][0], all_boxes[4][0], all_boxes[2][0] = rows(3), rows(2), rows(1)
    per = [R // 2, 1, R + 1 - R // 2 - 1]
    all_boxes[3][2], all_boxes[1][2], all_boxes[num_classes - 2][2] = rows(per[0]), rows(per[1]), rows(per[2])
    all_boxes[num_classes - 1][3] = rows(1)
    return all_boxes


def test_cells_to_padded_rows_to_cells_is_the_identity():
    from sniper_amd.mask_inference import image_rows, padded_passes, rows_to_cells
    rs = np.random.RandomState(0)
    NC, I, R = 9, 4, 6
    all_boxes = _synthetic_boxes(rs, NC, I, R)
    n_passes = []
    for i in range(I):
        boxes, cls, counts = image_rows(all_boxes, i)
        assert counts[0] == 0 and counts.sum() == len(boxes) == len(cls)
        assert (np.diff(cls) >= 0).all()                                  # class-major
        scale = 1.0 + 0.25 * i
        passes = padded_passes(boxes, cls, R, scale=scale, b=1)
        n_passes.append(len(passes))
        back_boxes, back_cls = [], []
        for rois, idx, valid in passes:
            assert rois.shape == (R, 5) and idx.shape == (R,) and rois.dtype == idx.dtype == np.float32
            assert (rois[:, 0] == 1).all() and (rois[valid:, 1:] == 0).all() and (idx[valid:] == 0).all()      # the padding rows
            back_boxes.append(rois[:valid, 1:] / np.float32(scale))
            back_cls.append(idx[:valid])
        if not passes:
            assert len(boxes) == 0
            continue
        cells = rows_to_cells(np.concatenate(back_boxes), counts)
        ccls = rows_to_cells(np.concatenate(back_cls), counts)
        for c in range(NC):
            want = np.asarray(all_boxes[c][i])[:, :4]
            assert cells[c].shape == want.shape
            assert np.allclose(cells[c], want, rtol=1e-6, atol=0)
            assert (ccls[c] == c - 1).all()
    assert n_passes == [1, 0, 2, 1]                                       # no detections: no pass; R + 1 rows: a second pass
    boxes, cls, counts = image_rows(all_boxes, 3)
    assert cls.tolist() == [NC - 2] and counts[NC - 1] == 1              # one detection in the last class: class index c - 1
    with pytest.raises(ValueError):
        padded_passes(boxes, cls, 0)
