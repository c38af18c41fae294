"""Base class of the network definitions (contract of the reference's symbols/symbol.py:9-61: `symbol`, `infer_shape` filling the
three name -> shape dictionaries, `check_parameter_shapes`, `get_msra_std`)."""
import numpy as np


def _shape_table(names, shapes):
    return {n: tuple(s) for n, s in zip(names, shapes)}


class Symbol(object):
    sym = None
    arg_shape_dict = out_shape_dict = aux_shape_dict = None

    symbol = property(lambda self: self.sym)

    def get_bbox_param_names(self):
        raise NotImplementedError()

    def infer_shape(self, data_shape_dict):
        g = self.sym
        inferred = g.infer_shape(**data_shape_dict)
        listings = (g.list_arguments(), g.list_outputs(), g.list_auxiliary_states())
        self.arg_shape_dict, self.out_shape_dict, self.aux_shape_dict = (_shape_table(n, s) for n, s in zip(listings, inferred))

    def ohem(self, cfg, score, bbox_pred, label, bbox_target, bbox_weight, num_classes):
        """Online hard example mining (TRAIN.ENABLE_OHEM; the wiring of the reference's symbols/faster/resnext_mx_101.py:311-332 over
        the native BoxAnnotatorOHEM operator): per image the TRAIN.BATCH_ROIS_OHEM RoIs of largest loss keep their label and box
        weights, every other RoI is ignored.  -> (label (R,) named `label_reshape`, bbox_weight (R, 4), number of RoIs per image
        that the box loss is normalised by).  Training graphs call this when cfg.TRAIN.get('ENABLE_OHEM') is set (.get: the
        reference's own config object may predate the keys); without the flag they build the graph they built before it existed."""
        import sniper_amd.mx as mx
        B, k = cfg.TRAIN.BATCH_IMAGES, int(cfg.TRAIN.get('BATCH_ROIS_OHEM', 256))
        per_image = lambda x, name, *tail: mx.sym.Reshape(data=x, shape=(B, -1) + tail, name=name)
        outs = mx.contrib.sym.BoxAnnotatorOHEM(
            name='box_annotator_ohem', num_classes=num_classes, num_reg_classes=1, roi_per_img=k,
            cls_score=per_image(score, 'ohem_cls_score', num_classes), bbox_pred=per_image(bbox_pred, 'ohem_bbox_pred', 4),
            labels=per_image(label, 'ohem_label'), bbox_targets=per_image(bbox_target, 'ohem_bbox_target', 4),
            bbox_weights=per_image(bbox_weight, 'ohem_bbox_weight', 4))
        return (mx.sym.Reshape(data=outs[0], shape=(-1,), name='label_reshape'),
                mx.sym.Reshape(data=outs[1], shape=(-1, 4), name='bbox_weight_reshape'), k)

    def get_msra_std(self, shape):
        """sqrt(2 / fan_in), fan_in = every dimension of the weight but the first (:36-41)."""
        return np.sqrt(2.0 / float(np.prod(shape[1:])))

    def check_parameter_shapes(self, arg_params, aux_params, data_shape_dict, is_train=True):
        """Every argument that is not an input (nor, at test time, a label) and every auxiliary state has a value of the inferred shape."""
        def verify(names, given, want):
            for k in names:
                assert k in given, k + ' not initialized'
                assert tuple(given[k].shape) == tuple(want[k]), 'shape inconsistent for %s: inferred %s, provided %s' % (
                    k, tuple(want[k]), tuple(given[k].shape))
        skip = lambda k: k in data_shape_dict or (not is_train and 'label' in k)
        verify([k for k in self.sym.list_arguments() if not skip(k)], arg_params, self.arg_shape_dict)
        verify(self.sym.list_auxiliary_states(), aux_params, self.aux_shape_dict)
