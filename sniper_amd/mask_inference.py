"""Mask prediction at test time: the trained mask head over an image's FINAL detections.

    all_boxes --MaskTester.predict / predict_masks--> all_masks --evaluation.evaluate_sds--> segm AP

The reference has no such stage (its lib/inference.py never mentions masks and the test branch of
symbols/faster/resnet_mx_101_e2e_mask.py:412-463 is the detector's), so the semantics here are this project's:

  * one scale per run: every image is resized as MNIteratorTest resizes it at `scale` (the same device image preparation,
    data/im_worker.py; the whole image, no FocusChips).  Routing a detection to a scale by its size, as VALID_RANGES does in training,
    is deliberately not done;
  * the rows of an image are its class cells in class-major order, boxes times the image's scale factor, class index c - 1, padded to
    `rois_per_image` rows with [b, 0, 0, 0, 0] / class 0 whose outputs are dropped; an image with more rows takes further passes of
    the same shape, an image without detections costs no pass;
  * batch shapes go through the Module's 64-pixel buckets and its shared activation pool (mx/module.py), so a run binds a handful
    of executors, not one per image;
  * the host does the row bookkeeping only (the functions below, plain numpy): 100 detections per image need no kernel.
"""
import numpy as np

import sniper_amd.mx as mx

MASK_SIZE = 28
# the default output stage of the mask test graph: the fused MaskClassProb operator (sn_mask_class_prob) or the stock chain.  Decided
# by measurement, profiles/mask_infer_bench.txt.
DEFAULT_FUSED = True


# ---------------------------------------------------------------------------------------------------------------------------------
# row bookkeeping (host, numpy only)
# ---------------------------------------------------------------------------------------------------------------------------------
def image_rows(all_boxes, i):
    """The detections of image i over all classes, class-major: -> (boxes (n,4) float64 in image pixels, cls (n,) class index c - 1,
    counts (len(all_boxes),) rows per class cell; class 0, the background, has none)."""
    boxes, cls, counts = [], [], np.zeros(len(all_boxes), np.int64)
    for c in range(1, len(all_boxes)):
        cell = all_boxes[c][i]
        cell = np.asarray(cell.cpu() if hasattr(cell, 'cpu') else cell, np.float64)
        if cell.size == 0:
            continue
        cell = cell.reshape(len(cell), -1)
        if cell.shape[1] < 4:
            raise ValueError('all_boxes[%d][%d] has %d columns: rows are x1, y1, x2, y2(, score)' % (c, i, cell.shape[1]))
        boxes.append(cell[:, :4])
        cls.append(np.full(len(cell), c - 1, np.int64))
        counts[c] = len(cell)
    if not boxes:
        return np.zeros((0, 4)), np.zeros((0,), np.int64), counts
    return np.concatenate(boxes), np.concatenate(cls), counts


def padded_passes(boxes, cls, rois_per_image, scale=1.0, b=0):
    """The rows of one image as network inputs: -> [(mask_rois (R,5) float32 rows [b, x1, y1, x2, y2] * scale, mask_cls (R,) float32,
    valid)] with R = rois_per_image -- ceil(n / R) passes of the same shape, none for n = 0; rows past `valid` are the padding
    [b, 0, 0, 0, 0] / class 0."""
    R = int(rois_per_image)
    if R < 1:
        raise ValueError('rois_per_image = %d' % R)
    out = []
    for lo in range(0, len(boxes), R):
        n = min(R, len(boxes) - lo)
        rois, idx = np.zeros((R, 5), np.float32), np.zeros((R,), np.float32)
        rois[:, 0] = b
        rois[:n, 1:] = np.asarray(boxes[lo:lo + n], np.float64) * float(scale)
        idx[:n] = cls[lo:lo + n]
        out.append((rois, idx, n))
    return out


def rows_to_cells(values, counts):
    """(n, ...) per-row values of one image in class-major order -> one array per class cell (`counts` of image_rows)."""
    values = np.asarray(values)
    assert len(values) == int(np.sum(counts)), (len(values), counts)
    edges = np.concatenate([[0], np.cumsum(counts)])
    return [values[edges[c]:edges[c + 1]] for c in range(len(counts))]


def _bucket64(n):
    return -(-int(n) // 64) * 64


# ---------------------------------------------------------------------------------------------------------------------------------
class MaskTester(object):
    """predict(roidb, all_boxes) -> all_masks, all_masks[c][i] = (n, 28, 28) float32 foreground probabilities, row for row the
    masks of all_boxes[c][i] ((0, 28, 28) for a cell without rows; all_masks[0] is the background's list of empties): what
    evaluation.evaluate_sds / COCOSegmEvaluator.convert_detections read.

    sym_inst: a resnet_mx_101_e2e_mask instance (its test_nbatch = images per forward); arg_params / aux_params: a training
    checkpoint's (the mask test graph's parameters are a subset); scale: (target, max), default the middle entry of cfg.TEST.SCALES;
    rois_per_image: rows per image and pass, default cfg.TEST.MAX_PER_IMAGE; module_cache (dict): keeps the bound Module across
    testers, like inference.detect_scale_worker's; fused: the output stage (None = DEFAULT_FUSED)."""

    def __init__(self, sym_inst, cfg, arg_params, aux_params, scale=None, rois_per_image=None, module_cache=None, fused=None,
                 context=None):
        self.cfg, self.sym_inst = cfg, sym_inst
        scales = list(cfg.TEST.SCALES)
        self.scale = tuple(int(v) for v in (scale if scale is not None else scales[len(scales) // 2]))
        per_image = cfg.TEST.get('max_per_image', cfg.TEST.get('MAX_PER_IMAGE', 100)) if rois_per_image is None else rois_per_image
        self.rois_per_image = int(per_image)
        self.nbatch = int(getattr(sym_inst, 'test_nbatch', 1))
        self.fused = DEFAULT_FUSED if fused is None else bool(fused)
        self.arg_params, self.aux_params = arg_params, aux_params
        self.context = context or [mx.gpu(0)]
        self._cache = module_cache if module_cache is not None else {}
        self._key = ('mask', self.scale, self.nbatch, self.rois_per_image, self.fused)
        self.module = self._cache.get(self._key)
        self._worker = None
        self.passes = 0              # forwards of the last predict()

    # ---- the bound network ------------------------------------------------------------------------------------------------
    def _shapes(self, hw):
        B, R = self.nbatch, self.rois_per_image
        return [('data', (B, 3, _bucket64(hw[0]), _bucket64(hw[1]))), ('mask_rois', (B * R, 5)), ('mask_cls', (B * R,))]

    def _module(self, hw):
        """the Module, bound at the first batch's shape (further shapes are the Module's own executors, one per 64-pixel bucket)"""
        if self.module is None:
            sym = self.sym_inst.get_symbol_mask_test(self.cfg, self.rois_per_image, fused=self.fused)
            mod = mx.mod.Module(symbol=sym, context=self.context, data_names=['data', 'mask_rois', 'mask_cls'], label_names=None)
            mod.slice_inputs = False
            mod.bind(self._shapes(hw), None, for_training=False)
            mod.init_params(arg_params=self.arg_params, aux_params=self.aux_params, allow_missing=self.arg_params is None)
            self.module = self._cache[self._key] = mod
        return self.module

    def bound_executors(self):
        return 0 if self.module is None else len(self.module._exes)

    # ---- images -----------------------------------------------------------------------------------------------------------
    def _prepare(self, r):
        """roidb entry -> ((3, h, w) float32 device tensor, the resized image; scale factor)"""
        import torch
        from . import hip
        from .data.im_worker import im_worker
        if self._worker is None:
            self._worker = im_worker(self.cfg, crop_size=None, target_size=self.scale)
        landscape = r['width'] >= r['height']
        canvas = [self.scale[0], self.scale[1]] if landscape else [self.scale[1], self.scale[0]]
        buf = torch.empty((3, canvas[0], canvas[1]), dtype=torch.float32, device=hip.require_gpu())
        scale, (h, w) = self._worker.worker([r['image'], canvas, r.get('flipped', False)], buf)
        return buf[:, :h, :w], float(scale)

    # ---- one forward ------------------------------------------------------------------------------------------------------
    def _forward(self, group, hw):
        """group: up to nbatch (image tensor, rois, cls, valid, sink) passes of one bucket shape"""
        import torch
        B, R = self.nbatch, self.rois_per_image
        if B == 1:
            data = group[0][0][None]
        else:                            # images of one bucket, zero padded to the largest (the Module pads on to the bucket)
            H, W = max(int(g[0].shape[1]) for g in group), max(int(g[0].shape[2]) for g in group)
            data = torch.zeros((B, 3, H, W), dtype=torch.float32, device=group[0][0].device)
            for b, g in enumerate(group):
                data[b, :, :g[0].shape[1], :g[0].shape[2]] = g[0]
        rois, cls = np.zeros((B * R, 5), np.float32), np.zeros((B * R,), np.float32)
        rois[:, 0] = np.repeat(np.arange(B), R)
        for b, g in enumerate(group):
            rois[b * R:(b + 1) * R], cls[b * R:(b + 1) * R] = g[1], g[2]
            rois[b * R:(b + 1) * R, 0] = b
        mod = self._module(hw)
        mod.forward(mx.io.DataBatch(data=[mx.nd.NDArray(data), mx.nd.array(rois), mx.nd.array(cls)], label=None), is_train=False)
        out = mod.get_outputs()[0].asnumpy()                      # (B * R, 1 | 2, 28, 28): copied before the next forward overwrites it
        prob = self.sym_inst.mask_prob_of(out)
        for b, g in enumerate(group):
            g[4].append(np.array(prob[b * R:b * R + g[3]], np.float32))
        self.passes += 1

    def predict(self, roidb, all_boxes):
        K1, I = len(all_boxes), len(roidb)
        for c in range(K1):
            if len(all_boxes[c]) != I:
                raise ValueError('all_boxes[%d] has %d images, the roidb %d' % (c, len(all_boxes[c]), I))
        empty = np.zeros((0, MASK_SIZE, MASK_SIZE), np.float32)
        all_masks = [[empty for _ in range(I)] for _ in range(K1)]
        self.passes = 0
        pending, sinks = {}, []              # bucket shape -> passes waiting for a full batch; (image, counts, its passes' outputs)
        for i, r in enumerate(roidb):
            boxes, cls, counts = image_rows(all_boxes, i)
            if not len(boxes):
                continue                     # no detections: no pass
            im, scale = self._prepare(r)
            sink = []
            sinks.append((i, counts, sink))
            hw = (_bucket64(im.shape[1]), _bucket64(im.shape[2]))
            for rois, idx, valid in padded_passes(boxes, cls, self.rois_per_image, scale):
                q = pending.setdefault(hw, [])
                q.append((im, rois, idx, valid, sink))
                if len(q) == self.nbatch:
                    self._forward(pending.pop(hw), hw)
        for hw in list(pending):
            self._forward(pending.pop(hw), hw)
        for i, counts, sink in sinks:
            cells = rows_to_cells(np.concatenate(sink), counts)
            for c in range(1, K1):
                if counts[c]:
                    all_masks[c][i] = cells[c]
        return all_masks


def predict_masks(sym_def, cfg, roidb, all_boxes, arg_params, aux_params, scale=None, rois_per_image=None, module_cache=None,
                  fused=None, nbatch=1, context=None):
    """The one-call form: sym_def is the symbol CLASS (symbols.faster.resnet_mx_101_e2e_mask.resnet_mx_101_e2e_mask), as
    inference.imdb_detection_wrapper takes it -> all_masks for evaluation.evaluate_sds(all_boxes, all_masks, roidb, num_classes)."""
    tester = MaskTester(sym_def(test_nbatch=nbatch), cfg, arg_params, aux_params, scale=scale, rois_per_image=rois_per_image,
                        module_cache=module_cache, fused=fused, context=context)
    return tester.predict(roidb, all_boxes)
