"""Generate tests/golden/cocoeval_v1.npz from the REFERENCE's own lib/dataset/pycocotools/cocoeval.py and maskApi.c (build
container only; the GPU box and the test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cocoeval_golden.py

How the reference is run (nothing translated or compiled is kept: it all lives in a temporary directory outside the repository):
  * cocoeval.py (Python 2) is copied there and lib2to3 is run on the copy;
  * the mechanical fixes a current numpy needs are applied to the copy: `np.float` -> `float`, and the two `np.round(...)+1`
    arguments of `np.linspace` in Params.__init__ are wrapped in `int(...)`;
  * the module `mask` it imports is a stub whose `iou` calls the reference's own bbIou: maskApi.c compiled with `gcc -shared` into
    the same directory, loaded with ctypes, the (n*m) result reshaped to (m, n) in Fortran order like _mask.pyx does;
  * the two COCO objects are a stand-in with getImgIds, getCatIds, getAnnIds, loadAnns over lists of annotation dicts
    (ids 1-based; detections carry iscrowd = 0 like COCO.loadRes gives them).

What the file holds, per set s in (small, large, hand) -- arrays only:
  s_shape = (K, I);  s_in_gt_* and s_in_dt_* the inputs (tests/coco_eval_util.py);  every evalImgs field with ids mapped to indices, in the
  flat layout of tests/coco_eval_ref.py: s_dt_rank (from dtIds), s_dt_scores, s_dt_match, s_dt_ignore, s_gt_match, s_gt_ignore
  (boxes put back from the reference's ignored-last order into arrival order);  s_precision, stored as (T,K,A,M,R) because the runs
  along R compress ten times better (the loader hands out the reference's (T,R,K,A,M));  s_recall;  s_stats.

Conditions asserted on the reference's own output: stats[0] within [0.2, 0.8] and >= 0.9 of the precision entries above -1 on the two
seeded sets; for every IoU threshold both matched and unmatched detections exist, in every set.
"""
import contextlib
import ctypes
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

import coco_eval_util as U  # noqa: E402
from oracle import build  # noqa: E402

PYCOCO = os.path.join(build.REF, 'lib', 'dataset', 'pycocotools')          # where the reference checkout lies (SNIPER_REFERENCE)

MASK_STUB = '''
import ctypes, numpy as np
_lib = None
def iou(dt, gt, iscrowd):
    m, n = len(dt), len(gt)
    if m == 0 or n == 0:
        return []
    d = np.ascontiguousarray(np.array(dt, dtype=np.double).reshape(m, 4))
    g = np.ascontiguousarray(np.array(gt, dtype=np.double).reshape(n, 4))
    c = np.ascontiguousarray(np.array(iscrowd, dtype=np.uint8))
    o = np.zeros((m * n,), dtype=np.double)
    P = ctypes.c_void_p
    _lib.bbIou(P(d.ctypes.data), P(g.ctypes.data), ctypes.c_ulong(m), ctypes.c_ulong(n), P(c.ctypes.data), P(o.ctypes.data))
    return o.reshape((m, n), order='F')
'''


class StandIn(object):
    """what COCOeval asks of a COCO object"""

    def __init__(self, anns, n_img, n_cat):
        self.anns, self.n_img, self.n_cat = anns, n_img, n_cat
        self.by_id = {a['id']: a for a in anns}

    def getImgIds(self):
        return list(range(1, self.n_img + 1))

    def getCatIds(self):
        return list(range(1, self.n_cat + 1))

    def getAnnIds(self, imgIds=[], catIds=[]):
        imgs, cats = set(imgIds), set(catIds)
        return [a['id'] for a in self.anns if (not imgs or a['image_id'] in imgs) and (not cats or a['category_id'] in cats)]

    def loadAnns(self, ids):
        return [self.by_id[i] for i in ids]


def load_reference(tmp):
    src = os.path.join(tmp, 'cocoeval.py')
    shutil.copy(os.path.join(PYCOCO, 'cocoeval.py'), src)
    subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', src], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(src) as fh:
        text = fh.read()
    assert text.count('np.float)') == 2 and text.count('np.round(') == 2
    text = text.replace('np.float)', 'float)')
    text = text.replace('np.round((0.95-.5)/.05)+1', 'int(np.round((0.95-.5)/.05)+1)')
    text = text.replace('np.round((1.00-.0)/.01)+1', 'int(np.round((1.00-.0)/.01)+1)')
    assert text.count('int(np.round(') == 2
    with open(src, 'w') as fh:
        fh.write(text)
    so = os.path.join(tmp, 'libmaskapi.so')
    subprocess.check_call(['gcc', '-shared', '-fPIC', '-O2', '-std=c99', '-I', PYCOCO, os.path.join(PYCOCO, 'maskApi.c'), '-o', so, '-lm'])
    with open(os.path.join(tmp, 'mask.py'), 'w') as fh:
        fh.write(MASK_STUB)
    sys.path.insert(0, tmp)
    sys.dont_write_bytecode = True
    import mask
    mask._lib = ctypes.CDLL(so)
    import cocoeval
    return cocoeval


def run_reference(cocoeval, gt, dt, K, I):
    gts = [dict(id=n + 1, image_id=int(gt['image'][n]) + 1, category_id=int(gt['category'][n]) + 1, bbox=[float(v) for v in gt['bbox'][n]],
                area=float(gt['area'][n]), iscrowd=int(gt['iscrowd'][n]), ignore=int(gt['ignore'][n])) for n in range(len(gt['image']))]
    dts = [dict(id=n + 1, image_id=int(dt['image'][n]) + 1, category_id=int(dt['category'][n]) + 1, bbox=[float(v) for v in dt['bbox'][n]],
                score=float(dt['score'][n]), area=float(dt['area'][n]), iscrowd=0) for n in range(len(dt['image']))]
    E = cocoeval.COCOeval(StandIn(gts, I, K), StandIn(dts, I, K))
    E.params.useSegm = 0
    with contextlib.redirect_stdout(io.StringIO()):
        E.evaluate()
        E.accumulate()
        E.summarize()
    p = E.params
    A, T = len(p.areaRng), len(p.iouThrs)
    gt_of, dt_of = {}, {}
    for g in gts:
        gt_of.setdefault((g['category_id'], g['image_id']), []).append(g['id'])
    for d in dts:
        dt_of.setdefault((d['category_id'], d['image_id']), []).append(d['id'])
    rank, scores, dtm, dtig, gtm, gtig = [], [], [], [], [], []
    for k in range(1, K + 1):
        for i in range(1, I + 1):
            es = [E.evalImgs[(k - 1) * A * I + a * I + (i - 1)] for a in range(A)]
            if es[0] is None:
                assert all(e is None for e in es) and (k, i) not in gt_of and (k, i) not in dt_of
                continue
            gids, dids = gt_of.get((k, i), []), dt_of.get((k, i), [])
            gpos = {g: n for n, g in enumerate(gids)}
            dpos = {d: n for n, d in enumerate(dids)}
            kept = es[0]['dtIds']
            krank = {d: r for r, d in enumerate(kept)}
            assert all(e['dtIds'] == kept and e['image_id'] == i and e['category_id'] == k for e in es)
            rank.append(np.array([dpos[d] for d in kept], np.int32))
            scores.append(np.array(es[0]['dtScores'], np.float64))
            m = np.zeros((A, T, len(kept)), np.int32)
            ig = np.zeros((A, T, len(kept)), np.uint8)
            gm = np.zeros((A, T, len(gids)), np.int32)
            gi = np.zeros((A, len(gids)), np.uint8)
            for a, e in enumerate(es):
                assert sorted(e['gtIds']) == gids
                cols = [gpos[g] for g in e['gtIds']]
                m[a] = np.vectorize(lambda v: 0 if v == 0 else gpos[int(v)] + 1, otypes=[np.int32])(e['dtMatches']).reshape(T, len(kept))
                ig[a] = np.asarray(e['dtIgnore']).reshape(T, len(kept)).astype(np.uint8)
                if gids:
                    gm[a][:, cols] = np.vectorize(lambda v: 0 if v == 0 else krank[int(v)] + 1, otypes=[np.int32])(e['gtMatches'])
                    gi[a, cols] = np.asarray(e['gtIgnore'], np.uint8)
            dtm.append(m), dtig.append(ig), gtm.append(gm), gtig.append(gi)
    cat = lambda arrs: np.concatenate(arrs, axis=-1)
    return dict(dt_rank=cat(rank), dt_scores=cat(scores), dt_match=cat(dtm), dt_ignore=cat(dtig), gt_match=cat(gtm), gt_ignore=cat(gtig),
                precision=E.eval['precision'], recall=E.eval['recall'], stats=np.asarray(E.stats, np.float64))


def main():
    assert os.path.isfile(os.path.join(PYCOCO, 'cocoeval.py')), 'the reference is not here: this script runs in the build container only'
    tmp = tempfile.mkdtemp(prefix='cocoeval_golden_')
    try:
        cocoeval = load_reference(tmp)
        out = {}
        for name, (gt, dt, K, I) in U.make_sets().items():
            res = run_reference(cocoeval, gt, dt, K, I)
            above = float(np.mean(res['precision'] > -1))
            print('%-5s K %2d I %3d boxes %4d detections %4d kept %4d  stats[0] %.4f  precision entries above -1: %.3f' % (
                name, K, I, len(gt['image']), len(dt['image']), len(res['dt_rank']), res['stats'][0], above))
            if name != 'hand':
                assert 0.2 <= res['stats'][0] <= 0.8, res['stats']
                assert above >= 0.9, above
            matched = res['dt_match'][0] != 0                       # area range 'all'
            assert matched.any(axis=1).all() and (~matched).any(axis=1).all(), 'a threshold lacks matched or unmatched detections'
            out['%s_shape' % name] = np.array([K, I], np.int32)
            for k in U.GT_KEYS:
                out['%s_in_gt_%s' % (name, k)] = gt[k]
            for k in U.DT_KEYS:
                out['%s_in_dt_%s' % (name, k)] = dt[k]
            for k in U.RESULT_KEYS:
                out['%s_%s' % (name, k)] = np.ascontiguousarray(res[k].transpose(0, 2, 3, 4, 1)) if k == 'precision' else res[k]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(U.GOLDEN, **out)
    print('wrote', U.GOLDEN, os.path.getsize(U.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
