"""CPU: grouped convolution (1 < num_group < channels) -- the lowering of the ResNeXt-101 graphs and of small grouped graphs without
launching kernels, the symbol's shapes and names, and the argument checks of the sn_gconv_* entry points."""
import ctypes
import re

import numpy as np
import pytest
import torch

import sniper_amd.mx as mx
from sniper_amd import config as cfgmod
from sniper_amd.engine.executor import Executor
from sniper_amd.symbols.faster import resnet_mx_101_e2e as r101
from sniper_amd.symbols.faster import resnext_mx_101_e2e as rx
from sniper_amd.train import fixed_param_names

B = 2
TRAIN_SHAPES = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, 21 * 32 * 32),
                    bbox_target=(B, 84, 32, 32), bbox_weight=(B, 84, 32, 32), gt_boxes=(B, 100, 5))
UNITS = (3, 4, 23, 3)
CG = {1: 4, 2: 8, 3: 16, 4: 32}


def _outputs(sym):
    """output names; an operator the graph builder named itself carries a process-wide counter (blockgrad0, blockgrad1, ...)"""
    return [re.sub(r'^(blockgrad)\d+', r'\1', n) for n in sym.list_outputs()]


@pytest.fixture(scope='module')
def train_ex():
    cfg = cfgmod.resnext101_e2e(batch_images=B)
    assert cfg.symbol == 'resnext_mx_101_e2e'
    sym = rx.resnext_mx_101_e2e(momentum=0.995).get_symbol_rcnn(cfg)
    return Executor(sym, TRAIN_SHAPES, True, fixed_param_names(cfg, sym), device=torch.device('cpu'))


def test_resnext_lowering_plan(train_ex):
    ex = train_ex
    convs = [s for s in ex.steps if type(s).__name__ == 'ConvolutionStep']
    grouped = [s for s in convs if s.grouped]
    assert len(grouped) == 33 and not any(s.depthwise for s in convs)
    assert not any(type(s).__name__ == 'DeformableConvolutionStep' for s in ex.steps)
    for s in grouped:
        stage = int(s.node.name[len('stage')])
        assert s.node.name.endswith('_conv2') and s.groups == 64 and s.C == s.O == 64 * CG[stage], s.node.name
        opener = s.node.name.endswith('unit1_conv2') and stage in (2, 3)
        assert s.s == ((2, 2) if opener else (1, 1)) and s.d == s.p == ((2, 2) if stage == 4 else (1, 1)), s.node.name
        # compact weights, read by the forward pass and the data gradient alike: no transposed copy
        assert s.w.int_shape == (s.O, 9, CG[stage]) and s.w.ref_shape == (s.O, CG[stage], 3, 3) and s.w.wT16 is None and not s.w.need_wT
        a = np.random.RandomState(stage).standard_normal(s.w.ref_shape).astype(np.float32)
        assert np.array_equal(s.w.to_reference(s.w.to_internal(a)), a)
        # none of the dense-only fusions
        assert s.stats_buf is None and s.dual_bn is None and s.fused_residual is None and s.b is None and not s.out_f32
        # frozen stage 1: no gradients; everything else trains
        assert s.y.needs_grad == (stage != 1) and s.w.trainable == (stage != 1), s.node.name
    assert sum(1 for s in grouped if s.node.name.startswith('stage3')) == 23
    # the BatchNorm behind a grouped layer takes its stand-alone statistics pass (stages 2 - 4); in the frozen stage 1 it is a
    # constant affine map behind a frozen layer and rides in the grouped layer's weights like behind a dense one
    bns = [s for s in ex.steps if type(s).__name__ == 'BatchNormStep' and getattr(s.x.producer, 'grouped', False)]
    assert len(bns) == 33 and all(s.stats_from is None and s.relu for s in bns)
    assert sorted(s.node.name for s in bns if s.folded_into is not None) == ['stage1_unit%d_bn2' % u for u in (1, 2, 3)]
    # the dense 1x1 layers around them keep their epilogue statistics
    assert all(s.stats_from is not None for s in ex.steps if type(s).__name__ == 'BatchNormStep' and s.node.name.startswith('stage3')
               and s.node.name.endswith(('_bn1', '_bn3')))
    for s in convs:
        if s.node.name == 'conv0' or s.node.name.startswith('stage1'):
            assert not s.y.needs_grad and not s.w.trainable
    assert sum(1 for p in ex.params.values() if p.trainable) == 30 * 9 + 3 * 3 + 9 * 2
    assert ex.params['stage3_unit5_conv2_weight'].half_region


def test_resnext_fix_bn_lowering_plan():
    """Trainer(fix_bn=True): every BatchNorm normalises with its moving statistics; behind a trainable grouped layer it stays a
    separate pass (nothing folds into a layer that trains)."""
    cfg = cfgmod.resnext101_e2e(batch_images=B)
    sym = rx.resnext_mx_101_e2e(momentum=0.995, fix_bn=True).get_symbol_rcnn(cfg)
    ex = Executor(sym, TRAIN_SHAPES, True, fixed_param_names(cfg, sym), device=torch.device('cpu'))
    bns = [s for s in ex.steps if type(s).__name__ == 'BatchNormStep' and getattr(s.x.producer, 'grouped', False)]
    assert len(bns) == 33 and all(s.global_stats and s.stats_from is None for s in bns)
    assert sum(1 for s in bns if s.folded_into is not None) == 3
    assert not any(s.stats_buf is not None for s in ex.steps if type(s).__name__ == 'ConvolutionStep' and s.grouped)


def test_resnext_test_graph_lowers():
    cfg = cfgmod.resnext101_e2e(batch_images=2)
    sym = rx.resnext_mx_101_e2e(test_nbatch=2).get_symbol_rcnn(cfg, is_train=False)
    ex = Executor(sym, dict(data=(2, 3, 512, 512), im_info=(2, 3), im_ids=(2,), chip_ids=(2,)), False, [], device=torch.device('cpu'))
    assert ex.n_trainable == 0 and any(type(s).__name__ == 'MultiProposalStep' for s in ex.steps)
    bns = [s for s in ex.steps if type(s).__name__ == 'BatchNormStep']
    folded = [s for s in bns if s.folded_into is not None]
    # post-activation units: every BatchNorm alone reads a convolution -- bn0, 33 x (bn1, bn2, bn3), 4 x sc_bn; bn_data is the stem
    assert len(bns) == 1 + 1 + 33 * 3 + 4 and len(folded) == len(bns) - 1
    assert sum(1 for s in folded if s.folded_into.grouped) == 33          # ... the grouped layers included (sn_gconv_fwd: bias + ReLU)
    assert all(s.folded_into.fold_bn is s and s.y.t is s.x.t for s in folded)


def test_grouped_deformable_convolution_raises_by_name():
    data, off = mx.sym.Variable('data'), mx.sym.Variable('offset')
    y = mx.contrib.sym.DeformableConvolution(data=data, offset=off, name='res5a_conv2', num_filter=16, kernel=(3, 3), pad=(1, 1),
                                             num_deformable_group=1, num_group=2, no_bias=True)
    with pytest.raises(NotImplementedError) as e:
        Executor(mx.sym.Group([y]), dict(data=(1, 16, 8, 8), offset=(1, 18, 8, 8)), False, [], device=torch.device('cpu'))
    assert 'res5a_conv2' in str(e.value) and 'num_group' in str(e.value)


def test_small_grouped_graphs_lower():
    """Cg != Og, a width off the fast path, a 5x5 kernel, a biased head-style layer with fp32 output: all lower to grouped steps;
    num_group == channels stays depthwise; a group count that does not divide the channels is refused by name."""
    data = mx.sym.Variable('data')
    a = mx.sym.Convolution(data=data, name='ga', num_filter=48, num_group=4, kernel=(3, 3), pad=(1, 1), no_bias=True)     # 6 -> 12
    b = mx.sym.Convolution(data=a, name='gb', num_filter=48, num_group=16, kernel=(5, 5), pad=(2, 2), no_bias=True)      # 3 -> 3
    c = mx.sym.Convolution(data=b, name='dw', num_filter=48, num_group=48, kernel=(3, 3), pad=(1, 1), no_bias=True)
    d = mx.sym.Convolution(data=c, name='gh', num_filter=8, num_group=2, kernel=(1, 1))                                   # bias, head
    ex = Executor(mx.sym.Group([d]), dict(data=(2, 24, 9, 7)), True, [], device=torch.device('cpu'))
    st = {s.node.name: s for s in ex.steps if type(s).__name__ == 'ConvolutionStep'}
    assert [(st[n].groups, st[n].grouped, st[n].depthwise) for n in ('ga', 'gb', 'dw', 'gh')] == \
        [(4, True, False), (16, True, False), (48, False, True), (2, True, False)]
    assert st['ga'].w.int_shape == (48, 9, 6) and st['gb'].w.int_shape == (48, 25, 3) and st['gh'].w.int_shape == (8, 1, 24)
    assert st['gh'].b is not None and st['gh'].out_f32 and all(s.w.wT16 is None for s in st.values())
    bad = mx.sym.Convolution(data=data, name='gbad', num_filter=48, num_group=5, kernel=(3, 3), pad=(1, 1), no_bias=True)
    with pytest.raises(Exception) as e:
        Executor(mx.sym.Group([bad]), dict(data=(2, 24, 9, 7)), True, [], device=torch.device('cpu'))
    assert 'gbad' in str(e.value) or 'num_group' in str(e.value)


def test_resnext_symbol_shapes_names_and_outputs():
    cfg = cfgmod.resnext101_e2e(batch_images=B)
    net, ref = rx.resnext_mx_101_e2e(momentum=0.995), r101.resnet_mx_101_e2e(momentum=0.995)
    assert (net.NUM_GROUP, net.MID, tuple(net.units)) == (64, 1.0, UNITS) and isinstance(net, r101.resnet_mx_101_e2e)
    sym, rsym = net.get_symbol_rcnn(cfg), ref.get_symbol_rcnn(cfgmod.res101_e2e(batch_images=B))
    assert _outputs(sym) == _outputs(rsym) and len(_outputs(sym)) == 5
    net.infer_shape(TRAIN_SHAPES)
    sd = net.arg_shape_dict
    for stage, shp in ((1, (256, 4, 3, 3)), (2, (512, 8, 3, 3)), (3, (1024, 16, 3, 3)), (4, (2048, 32, 3, 3))):
        for u in range(1, UNITS[stage - 1] + 1):
            assert tuple(sd['stage%d_unit%d_conv2_weight' % (stage, u)]) == shp
    assert tuple(sd['stage2_unit1_conv1_weight']) == (512, 256, 1, 1) and tuple(sd['stage2_unit1_sc_weight']) == (512, 256, 1, 1)
    want = set()
    for stage in (1, 2, 3, 4):
        for u in range(1, UNITS[stage - 1] + 1):
            p = 'stage%d_unit%d_' % (stage, u)
            layers = ['conv1', 'conv2', 'conv3'] + (['sc'] if u == 1 else [])
            bns = ['bn1', 'bn2', 'bn3'] + (['sc_bn'] if u == 1 else [])
            want |= {p + n + '_weight' for n in layers} | {p + n + s for n in bns for s in ('_gamma', '_beta')}
    args = set(sym.list_arguments())
    assert {n for n in args if n.startswith('stage')} == want
    heads = {n for n in set(rsym.list_arguments()) if not n.startswith('stage')}
    assert {n for n in args if not n.startswith('stage')} == heads
    aux = set(sym.list_auxiliary_states())
    assert {'stage2_unit1_sc_bn_moving_mean', 'stage4_unit3_bn3_moving_var', 'bn0_moving_mean'} <= aux
    # frozen through the existing FIXED_PARAMS: conv0, bn0, stage 1
    fixed = set(fixed_param_names(cfg, sym))
    assert {n for n in args if n.startswith(('stage1', 'conv0', 'bn0'))} <= fixed and not any(n.startswith('stage2') for n in fixed)
    # the head initialisation reaches every new layer and nothing of a trunk that has no offset branches
    arg, auxp = {}, {}
    net.init_weight_rcnn(cfg, arg, auxp)
    assert 'rpn_conv_3x3_weight' in arg and 'fc_new_1_weight' in arg and not any('stage' in n for n in arg)
    # the test graph: same outputs as the base class's
    tsym = rx.resnext_mx_101_e2e(test_nbatch=2).get_symbol_rcnn(cfg, is_train=False)
    assert _outputs(tsym) == _outputs(r101.resnet_mx_101_e2e(test_nbatch=2).get_symbol_rcnn(cfg, is_train=False))


# ---- C ABI: argument errors before any launch (no GPU here: nothing may be launched) ------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


def test_gconv_argument_errors_are_reported_before_any_launch(lib):
    from sniper_amd._lib import SniperHipError
    p = ctypes.c_void_p(16)

    def fwd(x=p, w=p, y=p, C=64, ips=64, O=64, ops=64, g=8, K=3):
        lib.call('sn_gconv_fwd', x, w, None, y, 1, 8, 8, C, ips, O, ops, g, K, K, 1, 1, 1, 0, 0, None)

    def dgrad(dy=p, C=64, O=64, dps=64, aps=64, xps=64, g=8, acc=None):
        lib.call('sn_gconv_dgrad', dy, p, acc, p, 1, 8, 8, C, O, dps, aps, xps, g, 3, 3, 1, 1, 1, None)

    def wgrad(dw=p, C=64, O=64, dps=64, xps=64, g=8, ws=p, nbytes=1 << 30):
        lib.call('sn_gconv_wgrad', p, p, dw, 1, 8, 8, C, O, dps, xps, g, 3, 3, 1, 1, 1, ws, nbytes, None)

    for call, word in ((lambda: fwd(x=None), 'null pointer'), (lambda: fwd(w=None), 'null pointer'), (lambda: fwd(y=None), 'null pointer'),
                       (lambda: dgrad(dy=None), 'null pointer'), (lambda: wgrad(dw=None), 'null pointer'),
                       (lambda: fwd(g=5), 'multiples of groups'), (lambda: fwd(O=60, ops=64, g=8), 'multiples of groups'),
                       (lambda: dgrad(C=60, g=8), 'multiples of groups'), (lambda: wgrad(O=36, g=8), 'multiples of groups'),
                       (lambda: fwd(ips=68), 'multiple of 8'), (lambda: fwd(ops=70), 'multiple of 8'),
                       (lambda: dgrad(dps=66), 'multiple of 8'), (lambda: dgrad(acc=p, aps=12), 'multiple of 8'),
                       (lambda: wgrad(xps=100), 'multiple of 8'), (lambda: fwd(ips=56), 'cover the channels'),
                       (lambda: fwd(g=1), 'dense'), (lambda: dgrad(g=1), 'dense'), (lambda: wgrad(g=1), 'dense'),
                       (lambda: fwd(g=64), 'depthwise'), (lambda: dgrad(g=64), 'depthwise'), (lambda: wgrad(g=64), 'depthwise'),
                       (lambda: wgrad(ws=None), 'sn_gconv_wgrad_workspace_bytes'), (lambda: wgrad(nbytes=16), 'sn_gconv_wgrad_workspace_bytes')):
        with pytest.raises(SniperHipError) as e:
            call()
        assert word in str(e.value), (word, str(e.value))


def test_gconv_wgrad_workspace_sizes(lib):
    raw = lib.raw
    q = raw('sn_gconv_wgrad_workspace_bytes')
    nw = 1024 * 9 * 16 * 4          # one fp32 partial slab of the stage-3 layer
    stage3 = q(20, 32, 32, 1024, 1024, 64, 3, 3, 1, 1, 1)
    assert stage3 > 0 and stage3 % nw == 0 and 1 <= stage3 // nw <= 512
    assert q(20, 128, 128, 256, 256, 64, 3, 3, 1, 1, 1) > 0 and q(20, 32, 32, 2048, 2048, 64, 3, 3, 1, 2, 2) > 0
    assert q(2, 11, 13, 24, 48, 4, 3, 3, 1, 1, 1) > 0                      # plain path
    assert q(2, 11, 13, 24, 48, 5, 3, 3, 1, 1, 1) == 0 and q(2, 11, 13, 24, 48, 1, 3, 3, 1, 1, 1) == 0 and q(2, 2, 2, 24, 48, 4, 5, 5, 1, 0, 1) == 0
