"""CPU: grouped deformable convolution (DeformableConvolution with num_group > 1) -- the lowering of small fast-path layers and of the
resnext_mx_101_e2e_dcn graphs without launching kernels, the refusal of every shape off the matrix-core path by name, and the
symbol's stage 4."""
import numpy as np
import pytest
import torch

import sniper_amd.mx as mx
from sniper_amd import config as cfgmod
from sniper_amd.engine.executor import Executor
from sniper_amd.symbols.faster import resnext_mx_101_e2e as rx
from sniper_amd.symbols.faster import resnext_mx_101_e2e_dcn as rxd
from sniper_amd.train import fixed_param_names

B = 2
TRAIN_SHAPES = dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, 21 * 32 * 32),
                    bbox_target=(B, 84, 32, 32), bbox_weight=(B, 84, 32, 32), gt_boxes=(B, 100, 5))
TEST_SHAPES = dict(data=(B, 3, 512, 512), im_info=(B, 3), im_ids=(B,), chip_ids=(B,))
CPU = torch.device('cpu')


def _layer(C, O, groups, dg, kernel=(3, 3), name='gd'):
    data, off = mx.sym.Variable('data'), mx.sym.Variable('off')
    pad = (kernel[0] // 2, kernel[1] // 2)
    return mx.contrib.sym.DeformableConvolution(data=data, offset=off, name=name, num_filter=O, kernel=kernel, pad=pad,
                                                num_deformable_group=dg, num_group=groups, no_bias=True)


def _shapes(C, dg, kernel=(3, 3)):
    return dict(data=(1, C, 6, 5), off=(1, 2 * kernel[0] * kernel[1] * dg, 6, 5))


def _step(ex):
    return [s for s in ex.steps if type(s).__name__ == 'DeformableConvolutionStep']


@pytest.mark.parametrize('for_training', [True, False])
def test_fast_path_layer_lowers_on_the_compact_weights(for_training):
    ex = Executor(_layer(64, 64, 2, 2), _shapes(64, 2), for_training, set(), device=CPU)
    (s,) = _step(ex)
    assert s.groups == 2 and s.dg == 2 and s.C == s.O == 64
    assert s.w.int_shape == (64, 9, 32) and s.w.ref_shape == (64, 32, 3, 3)
    a = np.random.RandomState(0).standard_normal(s.w.ref_shape).astype(np.float32)
    assert np.array_equal(s.w.to_reference(s.w.to_internal(a)), a)
    # no column buffer, no transposed copy of either kind, no split-K state used
    assert s.col is None and s.wT_flat is None and s.w.wT16 is None and not s.w.need_wT
    assert s.transpose_jobs() == [] and s.wT_flat is None
    assert s.b is None and not s.out_f32
    assert s.y.needs_grad == for_training


@pytest.mark.parametrize('C,O,groups,dg,kernel,word', [
    (64, 128, 2, 2, (3, 3), 'O / num_group'),          # Cg != Og
    (48, 48, 3, 1, (3, 3), 'C % 32'),                  # off the slab grid
    (64, 64, 2, 4, (3, 3), 'num_deformable_group'),    # a deformable group of 16 channels splits a slab
    (64, 64, 2, 2, (5, 5), '3x3'),                     # kernel
])
def test_shapes_off_the_fast_path_raise_by_name(C, O, groups, dg, kernel, word):
    for for_training in (True, False):
        with pytest.raises(NotImplementedError) as e:
            Executor(_layer(C, O, groups, dg, kernel, name='res5z_conv2'), _shapes(C, dg, kernel), for_training, set(), device=CPU)
        msg = str(e.value)
        assert 'res5z_conv2' in msg and 'num_group=%d' % groups in msg and word in msg, msg


def test_dense_deformable_step_keeps_its_column_path():
    ex = Executor(_layer(64, 64, 1, 2), _shapes(64, 2), True, set(), device=CPU)
    (s,) = _step(ex)
    assert s.groups == 1 and s.col is not None and s.col.shape == (30, 9 * 64) and s.w.need_wT and len(s.transpose_jobs()) == 1


@pytest.fixture(scope='module')
def dcn_cfg():
    cfg = cfgmod.resnext101_e2e_dcn(batch_images=B)
    assert cfg.symbol == 'resnext_mx_101_e2e_dcn'
    return cfg


def _check_stage4(ex, training):
    steps = _step(ex)
    assert [s.node.name for s in steps] == ['stage4_unit%d_conv2' % u for u in (1, 2, 3)]
    for s in steps:
        a = s.node.attrs
        assert s.groups == 64 and s.dg == 4 and s.C == s.O == 2048 and s.k == (3, 3) and s.s == (1, 1) and s.p == s.d == (2, 2)
        assert int(a['num_filter']) == 2048 and str(a.get('no_bias')) in ('True', '1', 'true') and s.b is None
        assert s.w.int_shape == (2048, 9, 32) and s.w.ref_shape == (2048, 32, 3, 3)
        assert s.col is None and s.wT_flat is None and not s.w.need_wT
        assert s.off.shape == (B, 72, 32, 32) and s.x.shape == (B, 2048, 32, 32)
        off = s.off.producer
        assert type(off).__name__ == 'ConvolutionStep' and off.node.name == s.node.name.replace('_conv2', '_offset')
        assert off.O == 72 and off.k == (3, 3) and off.p == off.d == (2, 2) and off.s == (1, 1) and off.b is not None and off.groups == 1
        assert str(off.node.attrs.get('cudnn_off')) in ('True', '1', 'true')
        assert off.x is s.x                                     # both read relu(bn1(conv1))
        assert s.x.producer.node.name.endswith('_relu1') or s.x.producer.node.name.endswith('_bn1')
        if training:
            assert s.w.trainable and off.w.trainable and off.b.trainable and s.y.needs_grad
    grouped = [s for s in ex.steps if type(s).__name__ == 'ConvolutionStep' and s.grouped]
    assert len(grouped) == 30 and not any(s.node.name.startswith('stage4') for s in grouped)


def test_dcn_symbol_training_graph_lowers(dcn_cfg):
    net = rxd.resnext_mx_101_e2e_dcn(momentum=0.995)
    sym = net.get_symbol_rcnn(dcn_cfg)
    ex = Executor(sym, TRAIN_SHAPES, True, fixed_param_names(dcn_cfg, sym), device=CPU)
    _check_stage4(ex, True)
    assert issubclass(rxd.resnext_mx_101_e2e_dcn, rx.resnext_mx_101_e2e)


def test_dcn_symbol_test_graph_lowers(dcn_cfg):
    sym = rxd.resnext_mx_101_e2e_dcn(test_nbatch=B).get_symbol_rcnn(dcn_cfg, is_train=False)
    ex = Executor(sym, TEST_SHAPES, False, set(), device=CPU)
    _check_stage4(ex, False)


def test_dcn_symbol_initialises_the_offset_layers_to_zero(dcn_cfg):
    net = rxd.resnext_mx_101_e2e_dcn(momentum=0.995)
    sym = net.get_symbol_rcnn(dcn_cfg)
    net.infer_shape(dict((k, v) for k, v in TRAIN_SHAPES.items()))
    args, aux = {}, {}
    net.init_weight_rcnn(dcn_cfg, args, aux)
    for u in (1, 2, 3):
        w, b = args['stage4_unit%d_offset_weight' % u], args['stage4_unit%d_offset_bias' % u]
        assert w.shape == (72, 2048, 3, 3) and b.shape == (72,)
        assert not np.asarray(w.asnumpy()).any() and not np.asarray(b.asnumpy()).any()
    assert net.arg_shape_dict['stage4_unit2_conv2_weight'] == (2048, 32, 3, 3)
    assert sym is not None


def test_plain_resnext_graph_is_unchanged():
    cfg = cfgmod.resnext101_e2e(batch_images=B)
    sym = rx.resnext_mx_101_e2e(momentum=0.995).get_symbol_rcnn(cfg)
    ex = Executor(sym, TRAIN_SHAPES, True, fixed_param_names(cfg, sym), device=CPU)
    assert sum(1 for s in ex.steps if type(s).__name__ == 'ConvolutionStep' and s.grouped) == 33
    assert not _step(ex)
