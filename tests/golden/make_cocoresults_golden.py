"""Generate tests/golden/cocoresults_v1.npz from the REFERENCE's own maskApi.c, lib/dataset/coco.py and lib/dataset/pascal_voc.py
(build container only; the GPU box and the test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cocoresults_golden.py

How the reference is run (as make_cocosegm_golden.py does; nothing translated or compiled is kept, it all lives in a temporary
directory outside the repository):
  * maskApi.c is compiled with `gcc -shared` and driven through ctypes: rleToString, rleFrString, rleEncode;
  * `coco_results_one_category_kernel` (coco.py:21-59) and `write_pascal_results` (pascal_voc.py:395-415) are cut out of their files by
    their `def` lines, go through lib2to3 (plus np.float -> float) and run against stand-ins: mask_voc2coco returns what
    pycocotools.mask.encode does for the bitmap it is handed (rleEncode + rleToString -- the resize is this project's own and is not
    pinned here), clip_boxes is the reference's arithmetic, `self` of the VOC writer holds classes, image_set_index and the template.

What the file holds -- arrays only:
  str_cnts + str_cnt_off   the count arrays of the string cases;  str_chars + str_off: the reference's rleToString of each (its
                           rleFrString gives the counts back: asserted here)
  det_rows + det_cell_off  the (n,5) float32 rows of all_boxes[k + 1][i], cell k * I + i;  det_image_ids, det_cat_ids, det_sizes
  det_cnts + det_cnt_off   the mask of every detection, as the reference's rleEncode of a random bitmap
  bbox_image / bbox_cat / bbox_box (n,4) / bbox_score            the reference's bbox records, in its order
  segm_image / segm_cat / segm_score / segm_chars + segm_off      the reference's segm records
  voc_chars + voc_off      the bytes of the VOC file of every class;  voc_images + voc_image_off, voc_classes + voc_class_off: names

The conditions that keep the reference defined, and the cases that must occur, are asserted in check().
"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import coco_segm_util as U  # noqa: E402
import make_cocosegm_golden as SEG  # noqa: E402
import rle_string_ref as R  # noqa: E402

GOLDEN = os.path.join(HERE, 'cocoresults_v1.npz')
LIB = os.path.dirname(os.path.dirname(SEG.PYCOCO))          # the reference's lib/
BOUNDARIES = (15, 16, -16, -17, 511, 512, -512, -513, 16383, 16384, 2 ** 19 - 1, 2 ** 19, 2 ** 24 - 1, 2 ** 24)
BASE = 2 ** 28
IMAGE_IDS, CAT_IDS = (11, 5, 42, 9, 27), (1, 3, 7, 90)
SIZES = ((40, 56), (33, 64), (48, 24), (20, 31), (37, 37))
VOC_IMAGES, VOC_CLASSES = ('000012', '000005', '2008_000042', '000009', '000027'), ('aeroplane', 'bicycle', 'bird', 'tvmonitor')


def string_cases(seed=5):
    """count arrays: one [1, 2^28, 2^28, 2^28 + x] per boundary and per width and sign (the fourth count codes x), the short masks, a
    first count of 0, and seeded arrays whose lengths straddle one and two chunks of the kernels"""
    rng = np.random.RandomState(seed)
    cases = [[1, BASE, BASE, BASE + x] for x in BOUNDARIES]
    for k in range(1, 7):
        lo, hi = (0 if k == 1 else 2 ** (5 * k - 6)), 2 ** (5 * k - 1)
        for sign in (1, -1):
            x = int(rng.randint(lo, hi))
            cases.append([1, BASE, BASE, BASE + (x if sign > 0 else -x - 1)])
    cases += [[1200], [7, 1193], [0, 5, 1195], [3, 40, 2, 1155], [0, 1, 1, 1, 1, 1196]]
    for m in (5, 31, 63, 64, 65, 66, 127, 128, 129, 130, 150, 191, 192, 193, 257):
        mag = rng.randint(0, 5, m)                                  # mixed magnitudes: every width below 2^28 occurs in a chain
        c = (rng.randint(0, 2 ** 31 - 1, m) % (32 ** (mag + 1) * 8)).astype(np.int64)
        c[0] = int(rng.randint(0, 16))                              # a one-character count: the reference's terminator fits
        cases.append(c.tolist())
    return [np.asarray(c, np.uint32) for c in cases]


def detections(seed=9):
    """all_boxes[k + 1][i] as float32 rows, with an image and a class that have no detection, exact halves at the rounded digit
    (multiples of 1/4 and 1/8, which float32 holds), and a bitmap per detection"""
    rng = np.random.RandomState(seed)
    K, I = len(CAT_IDS), len(IMAGE_IDS)
    cells, bitmaps = [], []
    for k in range(K):
        for i in range(I):
            h, w = SIZES[i]
            n = 0 if (k == 2 or i == 3) else int(rng.randint(0, 4))
            rows = np.zeros((n, 5), np.float32)
            for r in range(n):
                x1, y1 = rng.uniform(0, w - 2), rng.uniform(0, h - 2)
                x2, y2 = rng.uniform(x1, w - 1), rng.uniform(y1, h - 1)
                rows[r] = [x1, y1, x2, y2, rng.uniform(0.01, 1)]
                if rng.rand() < 0.4:
                    rows[r, :4] = np.round(rows[r, :4] * 8) / 8
                    rows[r, 4] = np.round(rows[r, 4] * 64) / 64
                bitmaps.append(U._blob(rng, h, w))
            cells.append(rows)
    return cells, bitmaps


def cut(path, start, stop):
    """the lines of `path` from the one that starts with `start` up to the one that starts with `stop`, dedented"""
    with open(path) as fh:
        lines = fh.read().split('\n')
    a = [n for n, ln in enumerate(lines) if ln.lstrip().startswith(start)][0]
    b = [n for n, ln in enumerate(lines) if n > a and ln.lstrip().startswith(stop)][0]
    pad = len(lines[a]) - len(lines[a].lstrip())
    return '\n'.join(ln[pad:] for ln in lines[a:b]) + '\n'


def translated(tmp, name, text):
    src = os.path.join(tmp, name)
    with open(src, 'w') as fh:
        fh.write(text)
    subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(src) as fh:
        return fh.read().replace('np.float)', 'float)')


def clip_boxes(boxes, im_shape):
    """lib/bbox/bbox_transform.py:35-50, restated for the stand-in (the segm records do not carry the box)"""
    boxes[:, 0::4] = np.maximum(np.minimum(boxes[:, 0::4], im_shape[1] - 1), 0)
    boxes[:, 1::4] = np.maximum(np.minimum(boxes[:, 1::4], im_shape[0] - 1), 0)
    boxes[:, 2::4] = np.maximum(np.minimum(boxes[:, 2::4], im_shape[1] - 1), 0)
    boxes[:, 3::4] = np.maximum(np.minimum(boxes[:, 3::4], im_shape[0] - 1), 0)
    return boxes


def check(cases, strings, cells, bbox, segm):
    """the conditions that keep the reference defined, and the cases the tests rely on"""
    seen = set()
    for c, s in zip(cases, strings):
        x = R.differences(c)
        k = R.widths(x)
        assert (np.abs(x) < 2 ** 29).all(), 'a difference of 2^29 or more: the reference overruns its six characters per count'
        assert (k < 6).any(), 'no count shorter than six characters: the reference\'s terminator may not fit'
        assert len(s) == int(k.sum()) and s == R.to_string(c)
        seen |= {(int(kk), bool(xx < 0)) for kk, xx in zip(k, x)}
    assert seen >= {(k, neg) for k in range(1, 7) for neg in (False, True)}, sorted(seen)
    xs = set(int(v) for c in cases for v in R.differences(c))
    assert set(BOUNDARIES) <= xs
    assert any(c[0] == 0 for c in cases) and {1, 2, 3, 4} <= {len(c) for c in cases}
    assert any(len(c) > 128 for c in cases)
    n = sum(len(c) for c in cells)
    assert len(bbox) == len(segm) == n and any(len(c) == 0 for c in cells)
    # the rounding is Python 3's (half to even, correctly rounded in decimal): the translated reference rounds numpy scalars, which
    # must agree with the builtin on every value chosen here
    rows = np.concatenate(cells).astype(np.float64)
    want = [[round(float(r[0]), 1), round(float(r[1]), 1), round(float(r[2] - r[0] + 1), 1), round(float(r[3] - r[1] + 1), 1)] for r in rows]
    assert [b['bbox'] for b in bbox] == want and [b['score'] for b in bbox] == [round(float(r[4]), 8) for r in rows]
    halves = sum(abs(abs(v * 10 - np.floor(v * 10)) - 0.5) < 1e-9 for r in rows for v in (r[0], r[1], r[2] - r[0] + 1, r[3] - r[1] + 1))
    assert halves >= 4, halves


def main():
    assert os.path.isfile(os.path.join(SEG.PYCOCO, 'maskApi.c')), 'the reference is not here: this script runs in the build container only'
    tmp = tempfile.mkdtemp(prefix='cocoresults_golden_')
    try:
        so = os.path.join(tmp, 'libmaskapi.so')
        subprocess.check_call(['gcc', '-shared', '-fPIC', '-O2', '-std=c99', '-I', SEG.PYCOCO, os.path.join(SEG.PYCOCO, 'maskApi.c'), '-o', so, '-lm'])
        api = SEG.MaskApi(so)
        cases = string_cases()
        strings = [api.to_string({'size': [1, int(c.sum(dtype=np.int64)) % (2 ** 31)], 'counts': c}) for c in cases]
        for c, s in zip(cases, strings):
            assert np.array_equal(api.plain({'size': [1, 1], 'counts': s})['counts'], c)
        cells, bitmaps = detections()
        K, I = len(CAT_IDS), len(IMAGE_IDS)
        masks = [api.encode(b) for b in bitmaps]
        # ---- COCO records
        ns = {'np': np, 'clip_boxes': clip_boxes, 'xrange': range,
              'mask_voc2coco': lambda ms, boxes, h, w, thr: [{'size': list(m['size']), 'counts': api.to_string(m)} for m in ms]}
        exec(translated(tmp, 'kernel.py', cut(os.path.join(LIB, 'dataset', 'coco.py'), 'def coco_results_one_category_kernel', 'class coco')), ns)
        info = [{'index': IMAGE_IDS[i], 'height': SIZES[i][0], 'width': SIZES[i][1]} for i in range(I)]
        off = np.concatenate([[0], np.cumsum([len(c) for c in cells])])
        bbox, segm = [], []
        for k in range(K):
            pack = {'cat_id': CAT_IDS[k], 'binary_thresh': 0.4, 'all_im_info': info, 'boxes': [cells[k * I + i] for i in range(I)],
                    'masks': [masks[off[k * I + i]:off[k * I + i + 1]] for i in range(I)]}
            bbox.extend(ns['coco_results_one_category_kernel'](dict(pack, ann_type='bbox')))
            segm.extend(ns['coco_results_one_category_kernel'](dict(pack, ann_type='segm')))
        check(cases, strings, cells, bbox, segm)
        # ---- VOC files
        vns = {}
        exec(translated(tmp, 'voc.py', cut(os.path.join(LIB, 'dataset', 'pascal_voc.py'), 'def write_pascal_results', 'def do_python_eval')), vns)

        class Self(object):
            classes = ('__background__',) + VOC_CLASSES
            image_set_index = VOC_IMAGES

            def get_result_file_template(self):
                return os.path.join(tmp, 'comp4_det_test_{:s}.txt')
        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            vns['write_pascal_results'](Self(), [[]] + [[cells[k * I + i] for i in range(I)] for k in range(K)])
        voc = []
        for cls in VOC_CLASSES:
            with open(os.path.join(tmp, 'comp4_det_test_%s.txt' % cls), 'rb') as fh:
                voc.append(fh.read())
        assert any(len(v) == 0 for v in voc) and sum(v.count(b'\n') for v in voc) == len(bbox)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = lambda items: (np.frombuffer(b''.join(items), np.uint8), np.concatenate([[0], np.cumsum([len(t) for t in items])]).astype(np.int32))
    out = {}
    out['str_cnts'], out['str_cnt_off'] = U.pool(cases)
    out['str_chars'], out['str_off'] = text([s.encode('ascii') for s in strings])
    out['det_rows'], out['det_cell_off'] = np.concatenate(cells).astype(np.float32), off.astype(np.int32)
    out['det_image_ids'], out['det_cat_ids'], out['det_sizes'] = np.array(IMAGE_IDS, np.int32), np.array(CAT_IDS, np.int32), np.array(SIZES, np.int32)
    out['det_cnts'], out['det_cnt_off'] = U.pool([m['counts'] for m in masks])
    out['bbox_image'], out['bbox_cat'] = np.array([b['image_id'] for b in bbox], np.int32), np.array([b['category_id'] for b in bbox], np.int32)
    out['bbox_box'], out['bbox_score'] = np.array([b['bbox'] for b in bbox], np.float64), np.array([b['score'] for b in bbox], np.float64)
    out['segm_image'], out['segm_cat'] = np.array([b['image_id'] for b in segm], np.int32), np.array([b['category_id'] for b in segm], np.int32)
    out['segm_score'] = np.array([b['score'] for b in segm], np.float64)
    out['segm_size'] = np.array([b['segmentation']['size'] for b in segm], np.int32)
    out['segm_chars'], out['segm_off'] = text([b['segmentation']['counts'].encode('ascii') for b in segm])
    out['voc_chars'], out['voc_off'] = text(voc)
    out['voc_images'], out['voc_image_off'] = text([s.encode('ascii') for s in VOC_IMAGES])
    out['voc_classes'], out['voc_class_off'] = text([s.encode('ascii') for s in VOC_CLASSES])
    np.savez_compressed(GOLDEN, **out)
    print('wrote %s, %d bytes: %d string cases (%d counts, %d characters), %d detections, %d VOC lines' % (
        GOLDEN, os.path.getsize(GOLDEN), len(cases), sum(len(c) for c in cases), sum(len(s) for s in strings), len(bbox),
        sum(v.count(b'\n') for v in voc)))


if __name__ == '__main__':
    main()
