"""Graph-level checks (CPU): our network definitions build on the mx shim, infer the BASELINE shapes,
and have exactly the arguments / auxiliary states / outputs / shapes / operator nodes that the reference's own
symbol file produces when run over the same shim (tests/golden/symbols_v1.json.gz, generated from the reference
itself by tests/golden/make_symbol_golden.py)."""
import os
import sys

import numpy as np
import pytest

from sniper_amd import config as cfgmod
from sniper_amd.symbols.faster import resnet_mx_101_e2e as ours

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
from make_symbol_golden import B as B_GOLDEN, MNV2_DEFAULTS, R_DEFAULTS, graph_signature, load  # noqa: E402


@pytest.fixture(scope='module')
def symbols_golden():
    return load()


def _same_graph(got, want):
    assert got['outputs'] == want['outputs']
    assert got['arguments'] == want['arguments'] and got['aux_states'] == want['aux_states']
    assert got['arg_shapes'] == want['arg_shapes'] and got['out_shapes'] == want['out_shapes']
    assert got.get('aux_shapes') == want.get('aux_shapes')
    # node-for-node: same operators with the same attributes (defaults dropped)
    assert len(got['nodes']) == len(want['nodes']) and got['nodes'] == want['nodes']


def _shapes(B, A=21, F=32, train=True):
    if train:
        return dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, A * F * F),
                    bbox_target=(B, 4 * A, F, F), bbox_weight=(B, 4 * A, F, F), gt_boxes=(B, 100, 5))
    return dict(data=(B, 3, 512, 512), im_info=(B, 3), im_ids=(B,), chip_ids=(B,))


def _cfg(B):
    cfg = cfgmod.res101_e2e(batch_images=B)
    cfg.TRAIN.ENABLE_OHEM = False
    return cfg


def test_r101_train_graph_shapes():
    B = 2
    cfg = _cfg(B)
    net = ours.resnet_mx_101_e2e(n_proposals=400, momentum=0.995)
    sym = net.get_symbol_rcnn(cfg)
    assert sym.list_outputs() == ['rpn_cls_prob_output', 'rpn_bbox_loss_output', 'cls_prob_reshape_output',
                                  'bbox_loss_reshape_output', 'blockgrad0_output']
    net.infer_shape(_shapes(B))
    assert net.out_shape_dict['rpn_cls_prob_output'] == (B, 2, 21 * 32, 32)
    assert net.out_shape_dict['cls_prob_reshape_output'] == (B, 300, 81)
    assert net.arg_shape_dict['conv0_weight'] == (64, 3, 7, 7)
    assert net.arg_shape_dict['rpn_conv_3x3_weight'] == (512, 3072, 3, 3)
    assert net.arg_shape_dict['fc_new_1_weight'] == (1024, 256 * 49)
    assert net.arg_shape_dict['stage4_unit1_offset_weight'] == (72, 512, 3, 3)
    n = sum(int(np.prod(s)) for k, s in net.arg_shape_dict.items() if k not in _shapes(B))
    assert abs(n / 1e6 - 73.7) < 0.1          # 73.5 M trainable + frozen stem
    params, aux = {}, {}
    net.init_weight_rcnn(cfg, params, aux)
    assert float(np.abs(params['offset_weight'].asnumpy()).sum()) == 0 and params['fc_new_1_weight'].shape == (1024, 12544)


def test_r101_test_and_rpn_graphs():
    cfg = _cfg(2)
    net = ours.resnet_mx_101_e2e(test_nbatch=2)
    sym = net.get_symbol_rcnn(cfg, is_train=False)
    assert sym.list_outputs() == ['rois_output', 'cls_prob_reshape_output', 'bbox_pred_reshape_output', 'im_ids', 'im_info',
                                  'chip_ids']
    net.infer_shape(_shapes(2, train=False))
    assert net.out_shape_dict['rois_output'] == (600, 5) and net.out_shape_dict['cls_prob_reshape_output'] == (2, 300, 81)
    cfg.TEST.AUTO_FOCUS = True
    sym = net.get_symbol_rcnn(cfg, is_train=False)
    assert 'scale_prob_output' in sym.list_outputs()
    rpn = net.get_symbol_rpn(_cfg(2))
    assert rpn.list_outputs() == ['rpn_cls_prob_output', 'rpn_bbox_loss_output']


@pytest.mark.parametrize('name', ['resnet_mx_101_e2e', 'resnet_mx_50_e2e'])
def test_same_graph_as_reference_symbol_file(symbols_golden, name):
    import importlib
    ourmod = importlib.import_module('sniper_amd.symbols.faster.' + name)
    for train in (True, False):
        want = symbols_golden['%s_%s' % (name, 'train' if train else 'test')]
        b = getattr(ourmod, name)(n_proposals=400, momentum=0.995, test_nbatch=B_GOLDEN)
        _same_graph(graph_signature(b, _cfg(B_GOLDEN), train, _shapes(B_GOLDEN, train=train), R_DEFAULTS), want)


def _mnv2_shapes(B, train=True, A=15, F=16):
    if train:
        return dict(data=(B, 3, 512, 512), valid_ranges=(B, 2), im_info=(B, 3), label=(B, A * F * F),
                    bbox_target=(B, 4 * A, F, F), bbox_weight=(B, 4 * A, F, F), gt_boxes=(B, 100, 5), crowd_boxes=(B, 10, 5))
    return dict(data=(B, 3, 512, 512), im_info=(B, 3), im_ids=(B,), chip_ids=(B,))


def test_mobilenetv2_graph_shapes():
    """BASELINE C1 network: 53 trunk convolutions (17 depthwise) + 4 head convolutions, stride-32 map, 15 anchors."""
    from sniper_amd.symbols.faster import mobilenetv2_e2e as mn
    B = 2
    cfg = cfgmod.mobilenetv2_e2e(batch_images=B)
    net = mn.mobilenetv2_e2e()
    sym = net.get_symbol_rcnn(cfg)
    assert sym.list_outputs() == ['rpn_cls_prob_output', 'rpn_bbox_loss_output', 'cls_prob_reshape_output',
                                  'bbox_loss_reshape_output', 'blockgrad0_output']
    net.infer_shape(_mnv2_shapes(B))
    assert net.out_shape_dict['rpn_cls_prob_output'] == (B, 2, 15 * 16, 16)
    assert net.out_shape_dict['cls_prob_reshape_output'] == (B, 300, 81)
    assert net.arg_shape_dict['first-3x3-conv-conv2d_weight'] == (32, 3, 3, 3)
    assert net.arg_shape_dict['seq-1-block0-depthwise-conv2d_weight'] == (96, 1, 3, 3)
    assert net.arg_shape_dict['last-1x1-conv-conv2d_weight'] == (1280, 320, 1, 1)
    assert net.arg_shape_dict['rpn_conv_3x3_weight'] == (256, 1280, 3, 3)
    assert net.arg_shape_dict['fc_new_1_weight'] == (512, 256 * 49)
    ops = [n for n in sym._topo() if n.op == 'Convolution']
    assert len(ops) == 53 + 4 and sum(1 for n in ops if int(n.attrs.get('num_group', 1)) > 1) == 17
    t = net.get_symbol_rcnn(cfg, is_train=False)
    assert t.list_outputs() == ['rois_output', 'cls_prob_reshape_output', 'bbox_pred_reshape_output', 'im_ids', 'im_info',
                                'chip_ids']


def test_mobilenetv2_same_graph_as_reference_symbol_file(symbols_golden):
    from sniper_amd.symbols.faster import mobilenetv2_e2e as mn
    for train in (True, False):
        want = symbols_golden['mobilenetv2_e2e_%s' % ('train' if train else 'test')]
        cfg = cfgmod.mobilenetv2_e2e(batch_images=B_GOLDEN)
        got = graph_signature(mn.mobilenetv2_e2e(test_nbatch=B_GOLDEN), cfg, train, _mnv2_shapes(B_GOLDEN, train), MNV2_DEFAULTS,
                              aux_shapes=False)
        _same_graph(got, want)


def _mask_shapes(B, train=True, A=21, F=32):
    d = _shapes(B, A, F, train)
    if train:
        d['gt_masks'] = (B, 100, 500)
    return d


def test_mask_graph_shapes():
    """configs/faster/sniper_res101_e2e_mask.yml network: RPN on C4, 6-output proposal target, 28x28 mask head."""
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    B = 2
    cfg = _cfg(B)
    net = mk.resnet_mx_101_e2e_mask(momentum=0.995)
    sym = net.get_symbol_rcnn(cfg)
    assert sym.list_outputs() == ['rpn_cls_prob_output', 'rpn_bbox_loss_output', 'cls_prob_reshape_output', 'bbox_loss_reshape_output',
                                  'blockgrad0_output', 'mask_cls_prob_output', 'blockgrad1_output']
    net.infer_shape(_mask_shapes(B))
    assert net.out_shape_dict['mask_cls_prob_output'] == (B * 50, 2, 28, 28) and net.out_shape_dict['blockgrad1_output'] == (B * 50, 28, 28)
    assert net.arg_shape_dict['rpn_conv_3x3_weight'] == (512, 1024, 3, 3)
    assert net.arg_shape_dict['mask_deconv_weight'] == (256, 256, 2, 2) and 'mask_deconv_bias' not in net.arg_shape_dict
    assert net.arg_shape_dict['mask_out_weight'] == (160, 256, 1, 1) and net.arg_shape_dict['mask_offset_weight'] == (392, 256 * 196)
    arg, aux = {}, {}
    net.init_weight_rcnn(cfg, arg, aux)
    assert float(np.abs(arg['mask_offset_weight'].asnumpy()).max()) == 0.0 and arg['mask_conv_3x3_4_weight'].shape == (256, 256, 3, 3)
    t = net.get_symbol_rcnn(cfg, is_train=False)
    assert t.list_outputs() == ['rois_output', 'cls_prob_reshape_output', 'bbox_pred_reshape_output', 'im_ids', 'im_info', 'chip_ids']


@pytest.mark.parametrize('autofocus', [False, True])
def test_mask_same_graph_as_reference_symbol_file(symbols_golden, autofocus):
    from sniper_amd.symbols.faster import resnet_mx_101_e2e_mask as mk
    for train in (True, False):
        want = symbols_golden['resnet_mx_101_e2e_mask%s_%s' % ('_autofocus' if autofocus else '', 'train' if train else 'test')]
        cfg = _cfg(B_GOLDEN)
        cfg.TRAIN.AUTO_FOCUS = cfg.TEST.AUTO_FOCUS = autofocus
        shp = _mask_shapes(B_GOLDEN, train)
        if autofocus and train:
            shp['scale_label'] = (B_GOLDEN, 1024)
        got = graph_signature(mk.resnet_mx_101_e2e_mask(momentum=0.995, test_nbatch=B_GOLDEN), cfg, train, shp, R_DEFAULTS, aux_shapes=False)
        _same_graph(got, want)
