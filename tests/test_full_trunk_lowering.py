"""CPU: network.FIXED_PARAMS = [] -- the stem and stage 1 of the ResNet-class graphs train through the max-pool backward.  The lowering
of R101, R50 and ResNeXt-101 without launching kernels, the C-ABI calls of an eager step with the recorder of
tests/golden/make_call_trace.py, Trainer's `fixed_params` plumbing, the argument checks of sn_maxpool_bwd and the compiler's resource
remarks of its kernel."""
import ctypes
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

from sniper_amd import config as cfgmod
from sniper_amd.engine.executor import Executor
from sniper_amd.train import fixed_param_names

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_call_trace import Recorder, trace  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2
SHAPES = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, 21 * 32 * 32),
              bbox_target=(B, 84, 32, 32), bbox_weight=(B, 84, 32, 32), gt_boxes=(B, 100, 5))
NETWORKS = {'resnet_mx_101_e2e': 'res101_e2e', 'resnet_mx_50_e2e': 'res101_e2e', 'resnext_mx_101_e2e': 'resnext101_e2e'}


def _symbol(name, fixed=None):
    cfg = getattr(cfgmod, NETWORKS[name])(batch_images=B)
    if fixed is not None:
        cfg.network.FIXED_PARAMS = list(fixed)
    cls = getattr(importlib.import_module('sniper_amd.symbols.faster.' + name), name)
    return cfg, cls(momentum=0.995).get_symbol_rcnn(cfg)


def _lower(name, fixed=None):
    cfg, sym = _symbol(name, fixed)
    return Executor(sym, SHAPES, True, fixed_param_names(cfg, sym), device=torch.device('cpu'))


def _pool(ex):
    pools = [s for s in ex.steps if type(s).__name__ == 'PoolingStep' and s.kind == 'max']
    assert len(pools) == 1
    return pools[0]


@pytest.mark.parametrize('name', sorted(NETWORKS))
def test_empty_fixed_params_lower_to_a_trainable_stem_and_stage1(name):
    ex = _lower(name, fixed=[])
    pool = _pool(ex)
    assert pool.x.needs_grad and pool.y.needs_grad and (pool.k, pool.s, pool.p) == ((3, 3), (2, 2), (1, 1))
    conv0 = [s for s in ex.steps if s.node.name == 'conv0'][0]
    assert conv0.is_stem and conv0.wkind == 'stem' and conv0.w.trainable and conv0.y.needs_grad
    # everything that is no input and not bn_data trains; bn_data stays folded into the image packing whatever the list says
    for n, p in ex.params.items():
        assert p.trainable == (not n.startswith('bn_data_')), n
    assert {'bn_data_gamma', 'bn_data_beta', 'conv0_weight', 'bn0_gamma', 'bn0_beta', 'stage1_unit1_conv1_weight'} <= set(ex.params)
    # both sides of conv0 -> bn0 and of the stage-1 pairs train: no BatchNorm rides in a convolution's weights
    bns = [s for s in ex.steps if type(s).__name__ == 'BatchNormStep']
    assert not any(s.folded_into is not None for s in bns)
    assert not any(getattr(s, 'fold_bn', None) is not None for s in ex.steps)
    # the reference's graph keeps bn0 and stage 1 on their moving statistics; their gamma / beta train
    low = [s for s in bns if s.node.name == 'bn0' or s.node.name.startswith('stage1_')]
    assert len(low) >= 1 + 3 * 3 and all(s.global_stats and s.gamma.trainable and s.beta.trainable and s.y.needs_grad for s in low)
    assert all(s.batched_refresh() for s in low)


@pytest.mark.parametrize('name', sorted(NETWORKS))
def test_the_configs_own_fixed_params_never_reach_the_pool_backward(name):
    ex = _lower(name)
    pool = _pool(ex)
    assert not pool.x.needs_grad and not pool.y.needs_grad
    assert not any(p.trainable for n, p in ex.params.items() if n.startswith(('conv0', 'bn0', 'bn_data', 'stage1_')))


def _called(phases):
    return {re.match(r'\s*(\w+)\(', line).group(1) for _, lines in phases for line in lines if re.match(r'\s*\w+\(', line)}


def test_eager_step_calls_with_the_configs_fixed_params(monkeypatch):
    """(holds before and after the kernel existed) the shipped R101 step never calls sn_maxpool_bwd"""
    names = _called(trace('resnet_mx_101_e2e/fix_bn=0', monkeypatch))
    assert 'sn_maxpool_fwd' in names and 'sn_conv_wgrad_batch' in names and 'sn_maxpool_bwd' not in names
    assert 'sn_conv_stem_wgrad' not in names


@pytest.mark.parametrize('defer', ['1', '0'])
def test_eager_step_calls_with_empty_fixed_params(monkeypatch, defer):
    """one eager R101 step with FIXED_PARAMS = [] on the recorder: one sn_maxpool_bwd on the pool's tensors, taking the first
    contribution to its input's gradient (no accumulate), the stem's weight gradient and bn0's frozen backward behind it"""
    from sniper_amd.mx import symbol as symmod
    for k in [k for k in os.environ if k.startswith('SNIPER_')]:
        monkeypatch.delenv(k)
    monkeypatch.setenv('SNIPER_WGRAD_DEFER', defer)
    symmod._counter().clear()
    rec = Recorder(monkeypatch)
    cfg, sym = _symbol('resnet_mx_101_e2e', fixed=[])
    rec.phase('setup')
    ex = Executor(sym, SHAPES, True, fixed_param_names(cfg, sym), device=torch.device('cpu'))
    rec.name_tensors(ex)
    ex.refresh_compute_copies()
    ex.is_train = True
    ex.load_inputs({k: np.zeros(v, np.float32) for k, v in SHAPES.items()})
    rec.name_tensors(ex)
    rec.phase('forward')
    ex._forward_body()
    rec.phase('backward')
    ex.backward()
    rec.phase('update')
    ex.update(0.01, 1e-4, 0.9, 1.0)
    back = [ln for ph, lines in rec.phases if ph == 'backward' for ln in lines]
    pool = [ln for ln in back if ln.startswith('sn_maxpool_bwd(')]
    assert len(pool) == 1, pool
    # dy (2,128,128,64), x = the fused bn0 + ReLU output (2,256,256,64), accumulate None, dx, N, H, W, C, k, stride, pad, stream
    assert re.match(r"sn_maxpool_bwd\(\S+:float16:\(2, 128, 128, 64\), val\.\S+:float16:\(2, 256, 256, 64\), None, "
                    r"\S+:float16:\(2, 256, 256, 64\), 2, 256, 256, 64, 3, 2, 1, None\)$", pool[0]), pool[0]
    at = back.index(pool[0])
    after = [re.match(r'\s*(\w+)\(', ln).group(1) for ln in back[at + 1:] if re.match(r'\s*\w+\(', ln)]
    assert 'sn_bn_frozen_backward' in after and 'sn_conv_stem_wgrad' in after
    # the stem computes no data gradient: nothing of the dgrad family follows bn0's backward
    assert not any(n.startswith('sn_conv_dgrad') for n in after[after.index('sn_bn_frozen_backward'):])


def test_trainer_fixed_params_reach_the_fixed_names():
    """Trainer(fixed_params=...) replaces cfg.network.FIXED_PARAMS, which fixed_param_names(cfg, sym) turns into Module's list (the
    plumbing only: Trainer itself needs a device)."""
    import inspect
    from sniper_amd.train import Trainer
    sig = inspect.signature(Trainer.__init__)
    assert sig.parameters['fixed_params'].default is None
    cfg, sym = _symbol('resnet_mx_101_e2e')
    own = fixed_param_names(cfg, sym)
    assert 'conv0_weight' in own and 'stage1_unit1_conv1_weight' in own and 'bn0_gamma' in own
    cfg, sym = _symbol('resnet_mx_101_e2e', fixed=[])
    assert fixed_param_names(cfg, sym) == []
    cfg, sym = _symbol('resnet_mx_101_e2e', fixed=['conv0'])
    assert fixed_param_names(cfg, sym) == ['conv0_weight']


def _stem_graph(kernel, stride, pad):
    import sniper_amd.mx as mx
    x = mx.sym.BatchNorm(data=mx.sym.Variable('data'), name='bn_data', fix_gamma=True, eps=2e-5, use_global_stats=True)
    x = mx.sym.Convolution(data=x, name='conv0', num_filter=64, kernel=(7, 7), stride=(2, 2), pad=(3, 3), no_bias=True)
    x = mx.sym.Activation(data=mx.sym.BatchNorm(data=x, name='bn0', fix_gamma=False, eps=2e-5, use_global_stats=True), act_type='relu')
    x = mx.sym.Pooling(data=x, kernel=kernel, stride=stride, pad=pad, pool_type='max', name='pool0')
    x = mx.sym.Convolution(data=x, name='head', num_filter=8, kernel=(1, 1), no_bias=True)
    return mx.sym.MakeLoss(data=x, name='loss')


@pytest.mark.parametrize('kernel, stride, pad', [((3, 3), (4, 4), (1, 1)), ((3, 3), (1, 1), (2, 2)), ((8, 8), (2, 2), (1, 1)),
                                                 ((3, 2), (2, 2), (1, 1)), ((3, 3), (2, 1), (1, 1)), ((3, 3), (2, 2), (1, 0))])
def test_a_pool_outside_the_backward_kernels_geometry_is_refused_at_lowering(kernel, stride, pad):
    """what sn_maxpool_bwd refuses, or a window that is not square: with a trainable stem below the pool the graph does not lower
    (not: lowers, runs forward and fails at the first backward); with the stem fixed the forward-only pool lowers as before"""
    sym, shapes = _stem_graph(kernel, stride, pad), dict(data=(1, 3, 64, 64))
    with pytest.raises(NotImplementedError, match='max-pool backward'):
        Executor(sym, shapes, True, [], device=torch.device('cpu'))
    ex = Executor(sym, shapes, True, ['conv0_weight', 'bn0_gamma', 'bn0_beta'], device=torch.device('cpu'))
    assert not _pool(ex).x.needs_grad
    ex = Executor(_stem_graph((3, 3), (1, 1), (1, 1)), shapes, True, [], device=torch.device('cpu'))
    assert _pool(ex).x.needs_grad


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


def test_maxpool_bwd_is_declared_and_exported(lib):
    ret, argtypes, argnames = lib.protos['sn_maxpool_bwd']
    assert argnames == ['dy', 'x', 'accumulate', 'dx', 'N', 'H', 'W', 'C', 'k', 'stride', 'pad', 'stream']
    assert ret is ctypes.c_int and argtypes[:4] == [ctypes.c_void_p] * 4 and argtypes[4:11] == [ctypes.c_int] * 7
    assert lib.raw('sn_maxpool_bwd') is not None
    with open(os.path.join(ROOT, 'include', 'sniper_hip.h')) as fh:
        header = fh.read()
    doc = header[header.index('Gradient of sn_maxpool_fwd'):header.index('int sn_maxpool_bwd(')]
    for word in ('row-major', 'FIRST', 'fp32', 'exactly once', 'no atomics', 'may alias dx', 'pad <= k / 2'):
        assert word in doc, word


def test_maxpool_bwd_argument_errors_are_reported_before_any_launch(lib):
    """(no GPU here: nothing may be launched, so every refusal below comes from the argument checks)"""
    from sniper_amd._lib import SniperHipError
    p = ctypes.c_void_p(16)

    def bwd(dy=p, x=p, acc=None, dx=p, N=1, H=8, W=8, C=16, k=3, s=2, pad=1):
        lib.call('sn_maxpool_bwd', dy, x, acc, dx, N, H, W, C, k, s, pad, None)

    for call, word in ((lambda: bwd(dy=None), 'null pointer'), (lambda: bwd(x=None), 'null pointer'), (lambda: bwd(dx=None), 'null pointer'),
                       (lambda: bwd(C=12), 'multiple of 8'), (lambda: bwd(C=0), 'multiple of 8'), (lambda: bwd(N=0), 'multiple of 8'),
                       (lambda: bwd(k=3, s=4), 'stride <= k'), (lambda: bwd(s=0), 'stride <= k'),
                       (lambda: bwd(k=3, s=1, pad=2), 'pad <= k / 2'), (lambda: bwd(k=2, s=2, pad=2), 'pad <= k / 2'),
                       (lambda: bwd(pad=-1), 'pad <= k / 2'), (lambda: bwd(k=8, s=2, pad=1), 'k <= 7'), (lambda: bwd(k=0, s=0, pad=0), 'k <= 7'),
                       (lambda: bwd(H=2, W=2, k=7, s=1, pad=1), 'does not fit')):
        with pytest.raises(SniperHipError) as e:
            call()
        assert 'sn_maxpool_bwd' in str(e.value) and word in str(e.value), (word, str(e.value))


def test_maxpool_bwd_kernel_resources():
    """The 3/2/1 kernel as planned: the 17 x 17 windows of a 32 x 32-pixel tile x 8 lanes x one 4-byte word of winner codes =
    9248 bytes of LDS, everything else in registers (no scratch, no spills), and at least two 256-thread workgroups per CU (a
    workgroup is one wave per SIMD, so waves per SIMD = workgroups per CU)."""
    from test_kernel_resources import _resources
    res = _resources('nn_ops')
    fast = {k: v for k, v in res.items() if 'maxpool_bwd_kernel' in k}
    plain = {k: v for k, v in res.items() if 'maxpool_bwd_plain_kernel' in k}
    assert len(fast) == 1 and len(plain) == 1, (sorted(fast), sorted(plain))
    for name, r in list(fast.items()) + list(plain.items()):
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['Occupancy'] >= 2, (name, r)
    (r,) = fast.values()
    assert r['LDS Size'] == 17 * 17 * 8 * 4 == 9248, r
    assert 160 * 1024 // r['LDS Size'] >= 2                      # ... and the LDS admits them too
    (r,) = plain.values()
    assert r['LDS Size'] == 0, r
