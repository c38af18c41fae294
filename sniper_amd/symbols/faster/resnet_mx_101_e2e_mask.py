"""ResNet-101 SNIPER with the auxiliary mask branch (configs/faster/sniper_res101_e2e_mask*.yml).

Same graph, parameter names and outputs as the reference's symbols/faster/resnet_mx_101_e2e_mask.py; the differences from
the plain R101 network (sniper_amd/symbols/faster/resnet_mx_101_e2e.py) are

  * the RPN reads the C4 features (cast to fp32) instead of concat(C4, C5)                      (:153-156, :291)
  * MultiProposalTargetMask also returns the 50 mask RoIs per chip and the GT row each one matched    (:317-318)
  * mask head (in the reference a training signal only: its test graph is the detector's):            (:238-254, :374-405)
      14x14 deformable PS-RoI pooling (+ its zero-initialised offset FC) -> 4 x [3x3 conv 256 + relu] -> 2x2/2
      deconvolution 256 + relu -> 1x1 conv to 2 x 80 maps at 28x28; MaskRcnnTarget rasterises the matched GT polygon
      into the RoI's 28x28 grid; `pick` takes the RoI class's negative / positive map -> 2-way per-pixel softmax.
  * get_symbol_mask_test (ours): the trained head over given boxes and classes -> (R, 1, 28, 28)
      foreground probabilities, the input of imdb.evaluate_sds; sniper_amd/mask_inference.py drives it.
"""
import numpy as np

import sniper_amd.mx as mx

from . import resnet_mx_101_e2e as base

checkpoint_callback = base.checkpoint_callback

MASK_SIZE, MASK_ROIS, MASK_CLASSES = 28, 50, 80


class resnet_mx_101_e2e_mask(base.resnet_mx_101_e2e):
    _NEW_MASK = tuple('mask_conv_3x3_%d' % (i + 1) for i in range(4)) + ('mask_out',)

    def get_rpn(self, feat, num_anchors):
        return base.resnet_mx_101_e2e.get_rpn(self, mx.sym.Cast(data=feat, dtype=np.float32), num_anchors)

    def _rpn(self, feat, cat, num_anchors):
        return self.get_rpn(feat, num_anchors)

    def _proposal_target(self, cfg, rpn_prob, box, im_info, gt_boxes, valid_ranges):
        return tuple(mx.sym.MultiProposalTargetMask(cls_prob=rpn_prob, bbox_pred=box, im_info=im_info, gt_boxes=gt_boxes,
                                                    valid_ranges=valid_ranges, batch_size=cfg.TRAIN.BATCH_IMAGES,
                                                    name='multi_proposal_target_mask'))

    def get_mask_features(self, feat, num_layers=4):
        """pooled (R, 256, 14, 14) features -> mask_deconv_relu (R, 256, 28, 28)"""
        x = feat
        for i in range(num_layers):
            x = mx.sym.Convolution(data=x, kernel=(3, 3), pad=(1, 1), num_filter=256, name='mask_conv_3x3_%d' % (i + 1))
            x = mx.sym.Activation(data=x, act_type='relu', name='mask_relu_%d' % (i + 1))
        x = mx.sym.Cast(data=x, dtype=np.float32)
        x = mx.sym.Deconvolution(data=x, kernel=(2, 2), stride=(2, 2), pad=(0, 0), num_filter=256, name='mask_deconv')
        return mx.sym.Activation(data=x, act_type='relu', name='mask_deconv_relu')

    def get_mask_head(self, feat, num_layers=4, num_classes=MASK_CLASSES):
        x = self.get_mask_features(feat, num_layers)
        return mx.sym.Convolution(data=x, kernel=(1, 1), pad=(0, 0), num_filter=num_classes * 2, name='mask_out')

    def _mask_pool(self, feat, mask_rois):
        """conv_new_1 features + RoIs -> 14x14 deformable PS-RoI pooled features (R, 256, 14, 14), cast to fp16 like the head"""
        pool = dict(group_size=1, pooled_size=14, sample_per_part=4, part_size=14, output_dim=256, spatial_scale=0.0625)
        t = mx.contrib.sym.DeformablePSROIPooling(name='mask_offset_t', data=feat, rois=mask_rois, no_trans=True, **pool)
        off = mx.sym.FullyConnected(name='mask_offset', data=t, num_hidden=14 * 14 * 2, lr_mult=0.01)
        off = mx.sym.Reshape(data=off, shape=(-1, 2, 14, 14), name='mask_offset_reshape')
        p = mx.contrib.sym.DeformablePSROIPooling(name='mask_deformable_roi_pool', data=feat, rois=mask_rois, trans=off,
                                                  no_trans=False, trans_std=0.1, **pool)
        return mx.sym.Cast(data=p, dtype=np.float16)

    def _extra_train_outputs(self, cfg, feat, extras, grad_scale):
        mask_rois, mask_ids = extras
        gt_masks = mx.sym.Variable(name='gt_masks')
        pred = self.get_mask_head(self._mask_pool(feat, mask_rois))
        targets, ncls = mx.sym.MaskRcnnTarget(rois=mask_rois, mask_polys=gt_masks, mask_ids=mask_ids,
                                              batch_size=cfg.TRAIN.BATCH_IMAGES, mask_size=MASK_SIZE, num_proposals=MASK_ROIS,
                                              max_polygon_len=500, max_num_gts=100, num_classes=MASK_CLASSES)
        pcls = ncls + MASK_CLASSES
        pos = mx.sym.pick(pred, index=pcls, axis=1, keepdims=True)
        neg = mx.sym.pick(pred, index=ncls, axis=1, keepdims=True)
        both = mx.sym.Concat(neg, pos, name='pred_cat')
        prob = mx.sym.SoftmaxOutput(data=both, label=targets, multi_output=True, normalization='valid', use_ignore=True,
                                    ignore_label=-1, name='mask_cls_prob', grad_scale=grad_scale)
        return [prob, mx.sym.BlockGrad(targets)]

    def get_mask_output(self, x, index, fused=True, num_classes=MASK_CLASSES):
        """mask_deconv_relu (R, 256, 28, 28) + one class index per RoI -> the foreground probability of each RoI's own class,
        float32.  fused: the one MaskClassProb operator (sn_mask_class_prob), (R, 1, 28, 28); otherwise the stock chain with the
        training graph's operators, (R, 2, 28, 28) = (background, foreground) -- the reference form of the tests, and what
        oracle/graph_cpu.py runs."""
        if fused:
            # (mask_out's parameters under their checkpoint names; the node itself is the graph's output `mask_prob`)
            return mx.contrib.sym.MaskClassProb(data=x, weight=mx.sym.Variable(name='mask_out_weight'),
                                                bias=mx.sym.Variable(name='mask_out_bias'), index=index, num_classes=num_classes,
                                                name='mask_prob')
        pred = mx.sym.Convolution(data=x, kernel=(1, 1), pad=(0, 0), num_filter=num_classes * 2, name='mask_out')
        pos = mx.sym.pick(pred, index=index + num_classes, axis=1, keepdims=True)
        neg = mx.sym.pick(pred, index=index, axis=1, keepdims=True)
        both = mx.sym.Concat(neg, pos, name='pred_cat')
        # (R, 2, 28, 28): the stock operators have no channel slice, so this form hands back both channels and its reader takes
        # channel 1 (mask_prob_of below)
        return mx.sym.SoftmaxActivation(data=both, mode='channel', name='mask_cls_prob')

    @staticmethod
    def mask_prob_of(out):
        """(R, 1 or 2, 28, 28) output of either form of the mask test graph -> (R, 28, 28) foreground probabilities"""
        return out[:, -1]

    def get_symbol_mask_test(self, cfg, rois_per_image=None, fused=True):
        """The mask test graph (ours; the reference's test graph is the detector's, :412-463): data, mask_rois (B * R, 5) rows
        [b, x1, y1, x2, y2] in pixels of the resized image, mask_cls (B * R,) class index per RoI -> mask_prob (B * R, 1, 28, 28).
        B = self.test_nbatch, R = rois_per_image (default cfg.TEST.max_per_image).  Trunk -> conv_new_1_relu -> the training graph's
        mask layers under the training graph's names, so its parameters are a subset of a training checkpoint's; no RPN, no detection
        head, no im_info."""
        data, rois, cls = (mx.sym.Variable(name=n) for n in ('data', 'mask_rois', 'mask_cls'))
        _, cat = self._trunk(cfg, data)
        feat = mx.sym.Activation(data=mx.sym.Convolution(data=cat, kernel=(1, 1), num_filter=256, name='conv_new_1'),
                                 act_type='relu', name='conv_new_1_relu')
        x = self.get_mask_features(self._mask_pool(feat, rois))
        self.sym = self.get_mask_output(x, cls, fused=fused)
        return self.sym

    def init_weight_mask(self, cfg, arg_params, aux_params):
        for n in self._NEW_MASK:
            arg_params[n + '_weight'] = mx.random.normal(0, 0.01, shape=self.arg_shape_dict[n + '_weight'])
            arg_params[n + '_bias'] = mx.nd.zeros(shape=self.arg_shape_dict[n + '_bias'])
        arg_params['mask_deconv_weight'] = mx.random.normal(0, 0.01, shape=self.arg_shape_dict['mask_deconv_weight'])
        self._init(arg_params, ['mask_offset'], 0)

    def init_weight_rcnn(self, cfg, arg_params, aux_params):
        base.resnet_mx_101_e2e.init_weight_rcnn(self, cfg, arg_params, aux_params)
        if 'mask_out_weight' in self.arg_shape_dict:      # the test graph has no mask head
            self.init_weight_mask(cfg, arg_params, aux_params)
