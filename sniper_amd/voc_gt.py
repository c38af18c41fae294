"""The ground truth of the VOC mask evaluation on the device (csrc/voc_gt.hip): the reference's parse_inst
(lib/dataset/pascal_voc_eval.py:275-318), the one stage between the SegmentationObject / SegmentationClass files and
evaluation.VOCSegmEvaluator that was missing.

    voc_instances(obj_maps, cls_maps)            index maps on the device -> per image the list of dicts parse_inst returns
    parse_inst_batch(image_names, devkit_path)   the files of a batch of images -> the same, through png_decode.decode_png(mode='index')

The host's share: one read-back of the per-id bounds, the running sum of the bitmaps' sizes, one download of the bitmaps."""
import os

import numpy as np

__all__ = ['voc_instances', 'parse_inst_batch']

IDS = 256
INST_FIELDS = 6
REC_FIELDS = 6
MAX_RECORDS = 65535          # csrc/voc_gt.hip: one launch's instances


def voc_instances(obj_maps, cls_maps, names=None):
    """obj_maps, cls_maps: per image an (h, w) uint8 map of instance ids / of classes (device tensors or arrays) -> one list per image
    of dicts with `mask` (bool, cropped to its bound), `mask_bound` (int [x1, y1, x2, y2]: min / max column / row) and `mask_cls`, in
    ascending instance id 1 .. 255 (id 0 is the background).  An instance whose pixels carry more than one class raises the
    reference's assertion, naming the image (names[i] where given) and the id; maps of unequal shape are a ValueError."""
    import torch
    from . import hip
    dev = hip.require_gpu()
    obj_maps, cls_maps = list(obj_maps), list(cls_maps)
    if len(obj_maps) != len(cls_maps):
        raise ValueError('voc_instances: %d object maps for %d class maps' % (len(obj_maps), len(cls_maps)))
    I = len(obj_maps)
    if I == 0:
        return []
    label = lambda i: repr(names[i]) if names is not None else '%d' % i
    objs, clss = [], []
    for i, (o, c) in enumerate(zip(obj_maps, cls_maps)):
        if tuple(o.shape) != tuple(c.shape):
            raise ValueError('voc_instances: image %s has an object map of shape %s and a class map of shape %s' % (label(i), tuple(o.shape), tuple(c.shape)))
        if len(o.shape) != 2 or min(int(o.shape[0]), int(o.shape[1])) < 1 or not str(o.dtype).endswith('uint8') or not str(c.dtype).endswith('uint8'):
            raise ValueError('voc_instances: (h, w) uint8 maps required, image %s has %s %s / %s' % (label(i), tuple(o.shape), o.dtype, c.dtype))
        objs.append(hip.dev(o))
        clss.append(hip.dev(c))
    out = []
    for start in range(0, I, 65535):
        out.extend(_instances(objs[start:start + 65535], clss[start:start + 65535], lambda i, s=start: label(s + i), dev))
    return out


def _instances(objs, clss, label, dev):
    import torch
    from . import hip
    I = len(objs)
    hw = np.array([[int(o.shape[0]), int(o.shape[1])] for o in objs], np.int32).reshape(I, 2)
    obj_ptrs = np.array([o.data_ptr() for o in objs], np.uint64)
    cls_ptrs = np.array([c.data_ptr() for c in clss], np.uint64)
    d_obj, d_cls, d_hw = hip.dev(obj_ptrs.view(np.int64)), hip.dev(cls_ptrs.view(np.int64)), hip.dev(hw)
    inst = torch.empty((I, IDS, INST_FIELDS), dtype=torch.int32, device=dev)
    st = hip.stream()
    hip.call('sn_vocgt_scan', d_obj, d_cls, d_hw, hw, I, inst, st)
    h_inst = inst.cpu().numpy()
    there = h_inst[:, :, 2] >= 0
    mixed = np.argwhere(there & (h_inst[:, :, 5] != 0))
    if len(mixed):
        i, k = int(mixed[0][0]), int(mixed[0][1])
        raise AssertionError('voc_instances: instance %d of image %s carries more than one class' % (k, label(i)))
    where = np.argwhere(there)          # (image, id), ascending in both
    N = len(where)
    records = [[] for _ in range(I)]
    if N == 0:
        return records
    rec = np.zeros((N, REC_FIELDS), np.int32)
    sel = h_inst[where[:, 0], where[:, 1]]
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = where[:, 0], where[:, 1], sel[:, 0], sel[:, 1]
    rec[:, 4], rec[:, 5] = sel[:, 2] - sel[:, 0] + 1, sel[:, 3] - sel[:, 1] + 1
    for a in range(0, N, MAX_RECORDS):
        r = np.ascontiguousarray(rec[a:a + MAX_RECORDS])
        n = len(r)
        off = np.zeros((n + 1,), np.int64)
        np.cumsum(r[:, 4].astype(np.int64) * r[:, 5], out=off[1:])
        pool = torch.empty((int(off[-1]),), dtype=torch.uint8, device=dev)
        hip.call('sn_vocgt_crop', d_obj, d_hw, hw, I, hip.dev(r), r, hip.dev(off), off, n, pool, int(off[-1]), st)
        bits = pool.cpu().numpy()
        for k in range(n):
            i, bw, bh = int(r[k, 0]), int(r[k, 4]), int(r[k, 5])
            s = sel[a + k]
            records[i].append({'mask': bits[off[k]:off[k + 1]].reshape(bh, bw).astype(bool),
                               'mask_cls': np.uint8(s[4]),
                               'mask_bound': np.array([s[0], s[1], s[2], s[3]], dtype=int)})
    return records


def parse_inst_batch(image_names, devkit_path):
    """the reference's parse_inst for a batch of images: SegmentationObject/<name>.png and SegmentationClass/<name>.png (8-bit palette
    files: their INDICES are read) decoded on the device -> records, one list per image, as evaluation.VOCSegmEvaluator and
    evaluate_sds_voc take them."""
    from .png_decode import decode_png
    image_names = list(image_names)
    obj = decode_png([os.path.join(devkit_path, 'SegmentationObject', n + '.png') for n in image_names], mode='index')
    cls = decode_png([os.path.join(devkit_path, 'SegmentationClass', n + '.png') for n in image_names], mode='index')
    return voc_instances(obj, cls, names=image_names)
