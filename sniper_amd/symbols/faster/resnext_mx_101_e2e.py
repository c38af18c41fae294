"""ResNeXt-101 (64 x 4d) Faster-RCNN for SNIPER, end to end: the trunk of the reference's symbols/faster/resnext_mx_101.py
(unit :69-127, num_group = 64 at :65, bottleneck width = num_filter at :89,98) under the RPN, heads, losses, test graph and
head initialisation of resnet_mx_101_e2e.py.

  unit:  conv1 1x1 -> bn1 relu -> conv2 3x3, num_group 64 -> bn2 relu -> conv3 1x1 -> bn3   (+ shortcut) -> relu
  shortcut: identity, or `_sc` 1x1 (stride of the unit) -> `_sc_bn`
  stage widths 256 / 512 / 1024 / 2048, units (3, 4, 23, 3): 4 / 8 / 16 / 32 channels per group in stages 1 - 4

Deviations from the reference file, which is dead upstream (no config names it, it imports a module that does not exist and its
test graph uses an undefined name), so the mirror is "its trunk under our e2e heads":
  * stage 4 is three units with a grouped DILATION-2 3x3 conv2 (stride 1, pad 2), what resnetc5(deform=False) builds for the dense
    trunk; the reference's stage 4 is a grouped deformable convolution (:161-168): resnext_mx_101_e2e_dcn.py builds that one.  The
    weight shape (2048, 32, 3, 3) is the reference's.
  * the shortcut BatchNorm's statistics mode follows its unit (moving statistics in the frozen stage 1 and under fix_bn, batch
    statistics otherwise); the reference has the two branches swapped at :119-122.
"""
import numpy as np

import sniper_amd.mx as mx

from . import resnet_mx_101_e2e as base

checkpoint_callback = base.checkpoint_callback


class resnext_mx_101_e2e(base.resnet_mx_101_e2e):
    NUM_GROUP = 64      # cardinality of conv2
    MID = 1.0           # bottleneck width / unit width (a 32 x 4d variant: NUM_GROUP = 32, MID = 0.5)

    def _unit(self, x, nf, stride, dim_match, name, frozen=False, deform=False, dilate=False):
        if deform:
            raise NotImplementedError('%s: the deformable stage 4 is resnext_mx_101_e2e_dcn' % name)
        mid = int(nf * self.MID)
        c1 = self._conv(x, name + '_conv1', mid, 1)
        a1 = self._bn_relu(c1, name, 1, frozen)
        pad = dil = 2 if dilate else 1
        c2 = mx.sym.Convolution(data=a1, name=name + '_conv2', num_filter=mid, num_group=self.NUM_GROUP, kernel=(3, 3),
                                stride=(stride, stride), pad=(pad, pad), dilate=(dil, dil), no_bias=True, workspace=self.workspace)
        a2 = self._bn_relu(c2, name, 2, frozen)
        c3 = self._conv(a2, name + '_conv3', nf, 1)
        b3 = self._bn(c3, name + '_bn3', frozen)
        sc = x if dim_match else self._bn(self._conv(x, name + '_sc', nf, 1, stride), name + '_sc_bn', frozen)
        return mx.sym.Activation(data=b3 + sc, act_type='relu', name=name + '_relu')

    def _trunk(self, cfg, data):
        feat = self.resnetc4(data, fp16=cfg.TRAIN.fp16)
        top = self.resnetc5(feat, deform=False)
        cat = mx.sym.Concat(feat, top, name='cat4')
        if cfg.TRAIN.fp16:
            cat = mx.sym.Cast(data=cat, dtype=np.float32)
        return feat, cat

    def init_weight_rpn(self, cfg, arg_params, aux_params):
        """no offset branches in this trunk; the `_sc_bn_*` layers are backbone layers (pretrained, or the Module's default
        initialisation like every other BatchNorm)"""
        self._init(arg_params, self._NEW_RPN, 0.01)
