"""Generate tests/golden/vocsds_v1.npz from the REFERENCE's own lib/dataset/pascal_voc_eval.py::voc_eval_sds and
lib/mask/mask_transform.py::mask_overlap (build container only; the GPU box and the test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vocsds_golden.py

How the reference is run (nothing translated is kept: it all lives in a temporary directory outside the repository):
  * pascal_voc_eval.py and mask/mask_transform.py (Python 2) are copied there and lib2to3 is run on the copies;
  * a stand-in `cv2` module is put beside them whose resize(src, (w, h)) is tests/coco_segm_ref.py::resize_linear_f32(src, h, w):
    the resize is specified by this project and NOT pinned to OpenCV, everything else is the reference's;
  * per set and class: the cache `<name>_mask_gt.pkl` the reference would write from the PNGs ({image name: [dict(mask, mask_cls,
    mask_bound, already_detect = False)]}, only images that have an instance of the class), so parse_inst / PIL are never reached;
    the detection pickle (a list over images of (n,5) rows), the mask pickle (a list over images of (n,M,M) maps), the image list;
  * voc_eval_sds(det_file, seg_file, devkit_path, image_list, cls_name, cache_dir, class_names, mask_size, binary_thresh, ov_thresh)
    is called per class at 0.5 and 0.7.

What the file holds, per set s in (small, edges, seeded) -- arrays only:
  s_shape = (K, I, M);  s_binary_thresh;  s_in_gt_* and s_in_dt_* the inputs (tests/voc_sds_ref.py);  s_ap (T,K) what voc_eval_sds returned.

Conditions asserted (on the restatement's intermediate results, after its AP has been found equal to the reference's on the bits):
the scores of every class are distinct; the mean AP at 0.5 of the seeded set lies within [0.2, 0.9]; the small and the seeded set have
matched and unmatched detections at both thresholds and a pair with an overlap strictly inside (0, 1) in every class; the edge set
holds every case its docstring lists."""
import contextlib
import io
import os
import pickle
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import voc_sds_ref as R  # noqa: E402
import voc_sds_util as U  # noqa: E402
from oracle import build  # noqa: E402

LIB = os.path.join(build.REF, 'lib')          # where the reference checkout lies (SNIPER_REFERENCE)

CV2_STAND_IN = '''
import os
import sys
sys.path.insert(0, %r)
from coco_segm_ref import resize_linear_f32


def resize(src, dsize):
    w, h = dsize
    return resize_linear_f32(src, int(h), int(w))
'''


def load_reference(tmp):
    os.mkdir(os.path.join(tmp, 'mask'))
    open(os.path.join(tmp, 'mask', '__init__.py'), 'w').close()
    shutil.copy(os.path.join(LIB, 'dataset', 'pascal_voc_eval.py'), os.path.join(tmp, 'pascal_voc_eval.py'))
    shutil.copy(os.path.join(LIB, 'mask', 'mask_transform.py'), os.path.join(tmp, 'mask', 'mask_transform.py'))
    for src in (os.path.join(tmp, 'pascal_voc_eval.py'), os.path.join(tmp, 'mask', 'mask_transform.py')):
        subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(os.path.join(tmp, 'cv2.py'), 'w') as fh:
        fh.write(CV2_STAND_IN % os.path.dirname(HERE))
    sys.path.insert(0, tmp)
    sys.dont_write_bytecode = True
    import pascal_voc_eval
    return pascal_voc_eval


def run_reference(ref, root, gt, dt, K, I, M, thr):
    """-> ap (T,K)"""
    os.makedirs(root)
    classes = ['__background__'] + ['class%02d' % k for k in range(K)]
    images = ['%06d' % i for i in range(I)]
    image_list = os.path.join(root, 'val.txt')
    with open(image_list, 'w') as fh:
        fh.write(''.join(name + '\n' for name in images))
    cache_dir = os.path.join(root, 'cache')
    os.mkdir(cache_dir)
    ap = np.zeros((len(U.THRESHOLDS), K))
    for k in range(K):
        name = classes[k + 1]
        s = dt['raw'][dt['category'] == k, 4]
        assert len(np.unique(s)) == len(s), 'class %d has equal scores' % k
        cache = {}
        for n in np.flatnonzero(gt['category'] == k):
            cache.setdefault(images[gt['image'][n]], []).append(
                {'mask': R.gt_mask(gt, n), 'mask_cls': k + 1, 'mask_bound': np.array(gt['bound'][n]), 'already_detect': False})
        with open(os.path.join(cache_dir, name + '_mask_gt.pkl'), 'wb') as fh:
            pickle.dump(cache, fh)
    for k in range(K):
        name = classes[k + 1]
        boxes, masks = [], []
        for i in range(I):
            sel = (dt['category'] == k) & (dt['image'] == i)
            boxes.append(dt['raw'][sel])
            masks.append(dt['masks'][sel])
        det_file, seg_file = os.path.join(root, name + '_det.pkl'), os.path.join(root, name + '_seg.pkl')
        with open(det_file, 'wb') as fh:
            pickle.dump(boxes, fh)
        with open(seg_file, 'wb') as fh:
            pickle.dump(masks, fh)
        for t, ov in enumerate(U.THRESHOLDS):
            with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide='ignore', invalid='ignore'):
                ap[t, k] = ref.voc_eval_sds(det_file, seg_file, root, image_list, name, cache_dir, classes, M, thr, ov)
    return ap


def pairs_of(want, p):
    D, G = want['dt_off'][p + 1] - want['dt_off'][p], want['gt_off'][p + 1] - want['gt_off'][p]
    return want['iou'][want['iou_off'][p]:want['iou_off'][p + 1]].reshape(D, G)


def assert_lively(name, want, K):
    """matched and unmatched detections at both thresholds, an overlap strictly inside (0, 1) in every class"""
    for k in range(K):
        c0, c1 = want['cls_off'][k], want['cls_off'][k + 1]
        for t in range(len(U.THRESHOLDS)):
            assert want['dt_tp'][t, c0:c1].any() and want['dt_fp'][t, c0:c1].any(), (name, k, t)
        ov = np.concatenate([pairs_of(want, p).reshape(-1) for p in range(want['cat_off'][k], want['cat_off'][k + 1])])
        assert ((ov > 0) & (ov < 1)).any(), (name, k)


def assert_edges(gt, dt, want):
    """every case tests/voc_sds_util.py::edges_set lists"""
    at = lambda i, k: np.flatnonzero((dt['image'] == i) & (dt['category'] == k))
    tp, fp, iou, box = want['dt_tp'], want['dt_fp'], want['dt_iou'], want['dt_box']
    n = at(0, 0)[0]
    assert iou[n] == 0.5 and tp[0, n] == 1 and fp[1, n] == 1                                  # exactly 0.5: tp under >=
    a, b = at(1, 0)
    assert iou[a] == 0.5 and want['dt_best'][a] == 1 and iou[b] == 1.0 and want['dt_best'][b] == 1     # two detections, one instance
    assert (tp[0, a], fp[0, b], fp[1, a], tp[1, b]) == (1, 1, 1, 1)
    assert want['dt_best'][at(2, 0)[0]] == 0 and iou[at(2, 0)[0]] == -1000.0                  # an image without instances of the class
    z = at(3, 0)[0]
    assert want['dt_area'][z] == 0 and iou[z] == 0.0 and want['dt_best'][z] == 1              # the all-zero map: union < 1
    assert want['npos'][3] == 0 and len(at(0, 3)) + len(at(7, 3)) == 2                        # detections, no instance anywhere
    assert want['npos'][4] == 1 and not (dt['category'] == 4).any()                           # an instance, no detections
    wh = np.stack((box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1), axis=1)[at(4, 1)].tolist()
    assert [1, 1] in wh and [12, 1] in wh and [1, 12] in wh and [2, 2] in wh                  # one pixel, one row, one column, exact 2x
    assert (box[at(4, 1), 0] < 0).any() and (box[at(4, 1), 2] < 0).any()                      # partly and wholly negative
    assert [0, 2, 4, 8] in box[at(4, 1)].tolist()                                             # halves to even
    assert want['dt_area'][at(5, 2)[0]] == 16 and want['dt_area'][at(6, 2)[0]] == 0           # on the threshold, one step below


def main():
    assert os.path.isfile(os.path.join(LIB, 'dataset', 'pascal_voc_eval.py')), 'the reference is not here: this script runs in the build container only'
    tmp = tempfile.mkdtemp(prefix='vocsds_golden_')
    try:
        ref = load_reference(tmp)
        out = {}
        for name, (gt, dt, K, I, M, thr) in U.make_sets().items():
            ap = run_reference(ref, os.path.join(tmp, name), gt, dt, K, I, M, thr)
            want = R.run(gt, dt, K, U.THRESHOLDS, thr)
            assert U.same_bits(want['ap07'], ap), (name, want['ap07'], ap)
            print('%-7s K %d I %2d M %2d instances %3d detections %4d pairs %4d  mean AP %.4f / %.4f' % (
                name, K, I, M, len(gt['image']), len(dt['image']), len(want['iou']), np.mean(ap[0]), np.mean(ap[1])))
            print(ap)
            if name == 'edges':
                assert_edges(gt, dt, want)
                assert np.isnan(want['rec'][:, want['cls_off'][3]:want['cls_off'][4]]).all() and (ap[:, 3] == 0).all() and (ap[:, 4] == 0).all()
            else:
                assert_lively(name, want, K)
            if name == 'seeded':
                assert 0.2 <= np.mean(ap[0]) <= 0.9, ap
            out['%s_shape' % name] = np.array([K, I, M], np.int32)
            out['%s_binary_thresh' % name] = np.float64(thr)
            for k in U.GT_KEYS:
                out['%s_in_gt_%s' % (name, k)] = gt[k]
            for k in U.DT_KEYS:
                out['%s_in_dt_%s' % (name, k)] = dt[k]
            out['%s_ap' % name] = ap
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(U.GOLDEN, **out)
    print('wrote', U.GOLDEN, os.path.getsize(U.GOLDEN), 'bytes')
    assert os.path.getsize(U.GOLDEN) <= 320 * 1000


if __name__ == '__main__':
    main()
