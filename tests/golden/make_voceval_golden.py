"""Generate tests/golden/voceval_v1.npz from the REFERENCE's own lib/dataset/pascal_voc_eval.py (build container only; the GPU box
and the test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_voceval_golden.py

How the reference is run (nothing translated is kept: it all lives in a temporary directory outside the repository):
  * pascal_voc_eval.py (Python 2) is copied there and lib2to3 is run on the copy;
  * the one mechanical fix a current numpy needs is applied to the copy: `np.bool` -> `bool`;
  * the module `mask.mask_transform` it imports (for the segmentation evaluation, not used here) is a stub;
  * per set: one XML annotation per image (object name, difficult, bndbox), the image-set file, and one result file per class in
    the format of write_pascal_results (lib/dataset/pascal_voc.py:412-415): '{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}' of the image
    name, the score and x + 1 taken on the float32 rows;
  * voc_eval(detpath, annopath, imageset_file, classname, annocache, ovthresh, use_07_metric) is called per class, threshold
    (0.5, 0.7) and metric.

What the file holds, per set s in (small, edges, voc_like) -- arrays only:
  s_shape = (K, I);  s_in_gt_* and s_in_dt_* the inputs (tests/voc_eval_util.py);  s_rows (ND,5) the result files read back the way
  voc_eval reads them;  s_cls_off (K+1);  s_rec, s_prec (T,ND): the reference's curves, class k's at [cls_off[k], cls_off[k+1]);
  s_ap07, s_ap_area (T,K).

Conditions asserted: the scores of every class are distinct after the 3-decimal rounding (the reference's order of equal scores is
undefined); rec and prec do not depend on the metric; the mean 11-point AP at 0.5 of the seeded sets lies within [0.2, 0.9]."""
import contextlib
import io
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import voc_eval_util as U  # noqa: E402
from oracle import build  # noqa: E402

DATASET = os.path.join(build.REF, 'lib', 'dataset')          # where the reference checkout lies (SNIPER_REFERENCE)

MASK_STUB = '''
def mask_overlap(*args):
    raise NotImplementedError('segmentation evaluation is not part of the box goldens')
'''


def load_reference(tmp):
    src = os.path.join(tmp, 'pascal_voc_eval.py')
    shutil.copy(os.path.join(DATASET, 'pascal_voc_eval.py'), src)
    subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(src) as fh:
        text = fh.read()
    assert text.count('np.bool)') == 1
    text = text.replace('np.bool)', 'bool)')
    with open(src, 'w') as fh:
        fh.write(text)
    os.mkdir(os.path.join(tmp, 'mask'))
    open(os.path.join(tmp, 'mask', '__init__.py'), 'w').close()
    with open(os.path.join(tmp, 'mask', 'mask_transform.py'), 'w') as fh:
        fh.write(MASK_STUB)
    sys.path.insert(0, tmp)
    sys.dont_write_bytecode = True
    import pascal_voc_eval
    return pascal_voc_eval


def write_inputs(root, gt, dt, K, I):
    """-> (detpath, annopath, imageset_file, class names, image names)"""
    os.makedirs(os.path.join(root, 'Annotations'))
    classes = ['class%02d' % k for k in range(K)]
    images = ['%06d' % i for i in range(I)]
    for i, name in enumerate(images):
        objs = []
        for n in np.flatnonzero(gt['image'] == i):
            b = gt['bbox'][n]
            assert (b == np.floor(b)).all()
            objs.append('<object><name>%s</name><difficult>%d</difficult><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax>'
                        '<ymax>%d</ymax></bndbox></object>' % (classes[gt['category'][n]], gt['difficult'][n], b[0], b[1], b[2], b[3]))
        with open(os.path.join(root, 'Annotations', name + '.xml'), 'w') as fh:
            fh.write('<annotation><filename>%s.jpg</filename>%s</annotation>\n' % (name, ''.join(objs)))
    imageset_file = os.path.join(root, 'test.txt')
    with open(imageset_file, 'w') as fh:
        fh.write(''.join(name + '\n' for name in images))
    # one result file per class, a line per detection in image order: name, score to 3 decimals, x + 1 (on the float32 row) to 1 decimal
    line = '{:s} {:.3f} {:.1f} {:.1f} {:.1f} {:.1f}\n'
    for k, cls in enumerate(classes):
        sel = np.flatnonzero(dt['category'] == k)
        assert dt['raw'].dtype == np.float32 and (np.diff(dt['image'][sel]) >= 0).all()
        with open(os.path.join(root, 'det_test_%s.txt' % cls), 'w') as fh:
            for n in sel:
                x1, y1, x2, y2, score = dt['raw'][n]
                fh.write(line.format(images[dt['image'][n]], score, x1 + 1, y1 + 1, x2 + 1, y2 + 1))
    return os.path.join(root, 'det_test_{:s}.txt'), os.path.join(root, 'Annotations', '{0!s}.xml'), imageset_file, classes, images


def read_rows(detpath, classes):
    """the result files the way voc_eval reads them -> (ND,5) float64 x1, y1, x2, y2, score, class-major"""
    rows = []
    for cls in classes:
        with open(detpath.format(cls)) as fh:
            for ln in fh:
                x = ln.strip().split(' ')
                rows.append([float(z) for z in x[2:]] + [float(x[1])])
    return np.array(rows, np.float64).reshape(-1, 5)


def run_reference(ref, root, gt, dt, K, I):
    detpath, annopath, imageset_file, classes, images = write_inputs(root, gt, dt, K, I)
    rows = read_rows(detpath, classes)
    assert len(rows) == len(dt['image'])
    cls_off = np.searchsorted(dt['category'], np.arange(K + 1)).astype(np.int32)
    for k in range(K):
        s = rows[cls_off[k]:cls_off[k + 1], 4]
        assert len(np.unique(s)) == len(s), 'class %d has equal scores after the rounding' % k
    T, ND = len(U.THRESHOLDS), len(rows)
    out = {'rows': rows, 'cls_off': cls_off, 'rec': np.zeros((T, ND)), 'prec': np.zeros((T, ND)), 'ap07': np.zeros((T, K)),
           'ap_area': np.zeros((T, K))}
    annocache = os.path.join(root, 'annotations.pkl')
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide='ignore', invalid='ignore'):
        for k, cls in enumerate(classes):
            for t, thr in enumerate(U.THRESHOLDS):
                rec, prec, ap07 = ref.voc_eval(detpath, annopath, imageset_file, cls, annocache, ovthresh=thr, use_07_metric=True)
                rec2, prec2, area = ref.voc_eval(detpath, annopath, imageset_file, cls, annocache, ovthresh=thr, use_07_metric=False)
                assert U.same_bits(np.asarray(rec, np.float64), np.asarray(rec2, np.float64)) and U.same_bits(np.asarray(prec, np.float64), np.asarray(prec2, np.float64))
                out['rec'][t, cls_off[k]:cls_off[k + 1]] = rec
                out['prec'][t, cls_off[k]:cls_off[k + 1]] = prec
                out['ap07'][t, k], out['ap_area'][t, k] = ap07, area
    return out


def main():
    assert os.path.isfile(os.path.join(DATASET, 'pascal_voc_eval.py')), 'the reference is not here: this script runs in the build container only'
    tmp = tempfile.mkdtemp(prefix='voceval_golden_')
    try:
        ref = load_reference(tmp)
        out = {}
        for name, (gt, dt, K, I) in U.make_sets().items():
            res = run_reference(ref, os.path.join(tmp, name), gt, dt, K, I)
            print('%-8s K %2d I %3d boxes %4d (%d difficult) detections %5d  mean AP07 %.4f / %.4f  mean area AP %.4f / %.4f' % (
                name, K, I, len(gt['image']), int(gt['difficult'].sum()), len(dt['image']), np.nanmean(res['ap07'][0]),
                np.nanmean(res['ap07'][1]), np.nanmean(res['ap_area'][0]), np.nanmean(res['ap_area'][1])))
            if name != 'edges':
                assert 0.2 <= np.mean(res['ap07'][0]) <= 0.9, res['ap07']
            out['%s_shape' % name] = np.array([K, I], np.int32)
            for k in U.GT_KEYS:
                out['%s_in_gt_%s' % (name, k)] = gt[k]
            for k in U.DT_KEYS:
                out['%s_in_dt_%s' % (name, k)] = dt[k]
            for k in U.GOLDEN_KEYS:
                out['%s_%s' % (name, k)] = res[k]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(U.GOLDEN, **out)
    print('wrote', U.GOLDEN, os.path.getsize(U.GOLDEN), 'bytes')
    assert os.path.getsize(U.GOLDEN) <= 320 * 1000


if __name__ == '__main__':
    main()
