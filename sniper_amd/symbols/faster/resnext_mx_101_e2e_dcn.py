"""ResNeXt-101 (64 x 4d) Faster-RCNN for SNIPER with the reference's deformable stage 4: resnext_mx_101_e2e with the three
stage-4 units of symbols/faster/resnext_mx_101.py:129-198 (residual_unit_deform).

  stage-4 unit:  conv1 1x1 -> bn1 relu -+-> `_offset` 3x3 (72 filters, pad 2, dilate 2, bias) -+
                                        +-> `_conv2` DeformableConvolution(2048, num_group 64,  <+   -> bn2 relu -> conv3 1x1 -> bn3
                                            num_deformable_group 4, 3x3, pad 2, dilate 2, stride 1, no bias)      (+ shortcut) -> relu

The grouped deformable convolution runs on the fused slab kernels of csrc/gdeform.hip.

Deviations from the reference file (dead upstream, see resnext_mx_101_e2e.py):
  * the shortcut BatchNorm's statistics mode follows its unit; the reference has the two branches swapped at :190-193, as at :119-122.
Deviation 1 of resnext_mx_101_e2e (a dilated stage 4 in place of the deformable one) is gone here.
"""
import numpy as np

import sniper_amd.mx as mx

from . import resnext_mx_101_e2e as base

checkpoint_callback = base.checkpoint_callback


class resnext_mx_101_e2e_dcn(base.resnext_mx_101_e2e):
    NUM_DEFORMABLE_GROUP = 4

    def _unit(self, x, nf, stride, dim_match, name, frozen=False, deform=False, dilate=False):
        if not deform:
            return base.resnext_mx_101_e2e._unit(self, x, nf, stride, dim_match, name, frozen, False, dilate)
        mid = int(nf * self.MID)
        c1 = self._conv(x, name + '_conv1', mid, 1)
        a1 = self._bn_relu(c1, name, 1, frozen)
        off = mx.sym.Convolution(data=a1, name=name + '_offset', num_filter=18 * self.NUM_DEFORMABLE_GROUP, kernel=(3, 3),
                                 stride=(1, 1), pad=(2, 2), dilate=(2, 2), cudnn_off=True)
        c2 = mx.contrib.sym.DeformableConvolution(data=a1, offset=off, name=name + '_conv2', num_filter=mid, kernel=(3, 3),
                                                  stride=(1, 1), pad=(2, 2), dilate=(2, 2), num_group=self.NUM_GROUP,
                                                  num_deformable_group=self.NUM_DEFORMABLE_GROUP, no_bias=True)
        a2 = self._bn_relu(c2, name, 2, frozen)
        c3 = self._conv(a2, name + '_conv3', nf, 1)
        b3 = self._bn(c3, name + '_bn3', frozen)
        sc = x if dim_match else self._bn(self._conv(x, name + '_sc', nf, 1, stride), name + '_sc_bn', frozen)
        return mx.sym.Activation(data=b3 + sc, act_type='relu', name=name + '_relu')

    def _trunk(self, cfg, data):
        feat = self.resnetc4(data, fp16=cfg.TRAIN.fp16)
        top = self.resnetc5(feat, deform=True)
        cat = mx.sym.Concat(feat, top, name='cat4')
        if cfg.TRAIN.fp16:
            cat = mx.sym.Cast(data=cat, dtype=np.float32)
        return feat, cat

    def init_weight_rpn(self, cfg, arg_params, aux_params):
        """the three `_offset` layers start at zero (resnet_mx_101_e2e.init_weight_rpn): the first steps sample the dilated lattice"""
        self._init(arg_params, ['stage4_unit%d_offset' % u for u in (1, 2, 3)], 0)
        base.resnext_mx_101_e2e.init_weight_rpn(self, cfg, arg_params, aux_params)
