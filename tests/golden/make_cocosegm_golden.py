"""Generate tests/golden/cocosegm_v1.npz from the REFERENCE's own lib/dataset/pycocotools/cocoeval.py and maskApi.c (build container
only; the GPU box and the test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_cocosegm_golden.py

How the reference is run (as make_cocoeval_golden.py does; nothing translated or compiled is kept, it all lives in a temporary
directory outside the repository):
  * maskApi.c is compiled with `gcc -shared` and driven through ctypes: rleEncode, rleFrPoly, rleMerge, rleArea, rleToBbox, rleIou,
    bbIou, rleToString, rleFrString;
  * cocoeval.py goes through lib2to3 with the same two numpy fixes, and runs with useSegm = 1;
  * the module `mask` it imports is a stand-in over those C functions (frPyObjects, merge, iou; the (n*m) result of rleIou reshaped
    to (m, n) in Fortran order like _mask.pyx does);
  * the two COCO objects are the stand-in of make_cocoeval_golden.py plus `imgs` (height and width per image); detections carry the
    area and bbox COCO.loadRes gives them (rleArea, rleToBbox) and iscrowd = 0.

What the file holds, per set s of tests/coco_segm_util.py (hand, edge, seeded) -- arrays only: s_shape = (K, I), s_sizes (I,2);
s_gt_image / category / area / iscrowd / ignore / form;  s_gt_cnts + s_gt_cnt_off: the reference's counts of every annotation (its
rleEncode of a bitmap, or rleFrPoly + rleMerge of the polygons);  s_gt_str + s_gt_str_off: the reference's rleToString where the
form is string counts;  s_poly_xy + s_poly_off + s_ann_poly_off: the polygons;  s_dt_image / category / score, s_dt_cnts +
s_dt_cnt_off, s_dt_area, s_dt_bbox;  s_iou + s_iou_off: rleIou of every problem, detection-major in arrival order;  the evalImgs
fields in the flat layout of tests/coco_eval_ref.py as s_res_*, precision (stored (T,K,A,M,R)), recall, stats.

Conditions asserted on the reference's own output are in check() below.
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
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import coco_segm_util as U  # noqa: E402
import make_cocoeval_golden as BOX  # noqa: E402

PYCOCO = BOX.PYCOCO
P = ctypes.c_void_p

MASK_STUB = '''
_impl = None
def frPyObjects(objs, h, w):
    return _impl.frPyObjects(objs, h, w)
def merge(rles):
    return _impl.merge(rles)
def iou(dt, gt, iscrowd):
    return _impl.iou(dt, gt, iscrowd)
'''


class RLE(ctypes.Structure):
    _fields_ = [('h', ctypes.c_ulong), ('w', ctypes.c_ulong), ('m', ctypes.c_ulong), ('cnts', ctypes.POINTER(ctypes.c_uint))]


class MaskApi(object):
    """maskApi.c through ctypes; a mask on the Python side is {'size': [h, w], 'counts': uint32 array}"""

    def __init__(self, so):
        self.c = ctypes.CDLL(so)
        self.c.rleToString.restype = ctypes.c_void_p

    def _in(self, rles):
        arr = (RLE * len(rles))()
        keep = []
        for r, o in zip(arr, rles):
            o = self.plain(o)
            c = np.ascontiguousarray(o['counts'], np.uint32)
            keep.append(c)
            r.h, r.w, r.m = o['size'][0], o['size'][1], len(c)
            r.cnts = c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))
        return arr, keep

    @staticmethod
    def _out(r):
        return {'size': [int(r.h), int(r.w)], 'counts': np.array([r.cnts[j] for j in range(r.m)], np.uint32)}

    def plain(self, o):
        """string counts -> counts through the reference's rleFrString"""
        if isinstance(o['counts'], str):
            r = RLE()
            self.c.rleFrString(ctypes.byref(r), ctypes.c_char_p(o['counts'].encode('ascii')), ctypes.c_ulong(o['size'][0]), ctypes.c_ulong(o['size'][1]))
            out = self._out(r)
            self.c.rleFree(ctypes.byref(r))
            return out
        return o

    def encode(self, bitmap):
        h, w = bitmap.shape
        flat = np.ascontiguousarray(np.asarray(bitmap, np.uint8).T).reshape(-1)
        r = RLE()
        self.c.rleEncode(ctypes.byref(r), P(flat.ctypes.data), ctypes.c_ulong(h), ctypes.c_ulong(w), ctypes.c_ulong(1))
        out = self._out(r)
        self.c.rleFree(ctypes.byref(r))
        return out

    def to_string(self, o):
        arr, keep = self._in([o])
        p = self.c.rleToString(ctypes.byref(arr[0]))
        return ctypes.string_at(p).decode('ascii')

    def fr_poly(self, xy, h, w):
        xy = np.ascontiguousarray(xy, np.float64)
        r = RLE()
        self.c.rleFrPoly(ctypes.byref(r), P(xy.ctypes.data), ctypes.c_ulong(len(xy) // 2), ctypes.c_ulong(h), ctypes.c_ulong(w))
        out = self._out(r)
        self.c.rleFree(ctypes.byref(r))
        return out

    def frPyObjects(self, objs, h, w):
        out = []
        for o in objs:
            if isinstance(o, dict):                   # uncompressed counts
                out.append({'size': [h, w], 'counts': np.asarray(o['counts'], np.uint32)})
            else:
                out.append(self.fr_poly(o, h, w))
        return out

    def merge(self, rles, intersect=0):
        arr, keep = self._in(rles)
        r = RLE()
        self.c.rleMerge(arr, ctypes.byref(r), ctypes.c_ulong(len(rles)), ctypes.c_bool(bool(intersect)))
        out = self._out(r)
        self.c.rleFree(ctypes.byref(r))
        return out

    def area(self, o):
        arr, keep = self._in([o])
        a = ctypes.c_uint(0)
        self.c.rleArea(arr, ctypes.c_ulong(1), ctypes.byref(a))
        return int(a.value)

    def bbox(self, o):
        arr, keep = self._in([o])
        bb = np.zeros(4, np.float64)
        self.c.rleToBbox(arr, P(bb.ctypes.data), ctypes.c_ulong(1))
        return bb

    def bb_iou(self, d, g):
        o = np.zeros(1, np.float64)
        d, g = np.ascontiguousarray(d, np.float64), np.ascontiguousarray(g, np.float64)
        self.c.bbIou(P(d.ctypes.data), P(g.ctypes.data), ctypes.c_ulong(1), ctypes.c_ulong(1), None, P(o.ctypes.data))
        return float(o[0])

    def iou(self, dt, gt, iscrowd):
        m, n = len(dt), len(gt)
        if m == 0 or n == 0:
            return []
        da, k1 = self._in(dt)
        ga, k2 = self._in(gt)
        c = np.ascontiguousarray(np.array(iscrowd, dtype=np.uint8))
        o = np.zeros((m * n,), dtype=np.double)
        self.c.rleIou(da, ga, ctypes.c_ulong(m), ctypes.c_ulong(n), P(c.ctypes.data), P(o.ctypes.data))
        return o.reshape((m, n), order='F')


class StandIn(BOX.StandIn):
    def __init__(self, anns, n_img, n_cat, sizes):
        BOX.StandIn.__init__(self, anns, n_img, n_cat)
        self.imgs = {i + 1: {'height': int(sizes[i][0]), 'width': int(sizes[i][1])} for i in range(n_img)}


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
    api = MaskApi(so)
    mask._impl = api
    import cocoeval
    return cocoeval, api


def run_reference(cocoeval, api, s):
    K, I, sizes = s['K'], s['I'], s['sizes']
    gts, gt_rle, forms, strings, polys = [], [], [], [], []
    for n, a in enumerate(s['gt']):
        h, w = (int(v) for v in sizes[a['image']])
        kind, val = a['seg']
        if kind == 'poly':
            seg = [list(p) for p in val]
            parts = api.frPyObjects(seg, h, w)
            rle = parts[0] if len(parts) == 1 else api.merge(parts)
            forms.append(U.FORM_POLY), strings.append(''), polys.append(val)
        else:
            rle = api.encode(val)
            text = api.to_string(rle) if kind == 'string' else ''
            assert np.array_equal(api.plain({'size': [h, w], 'counts': text})['counts'], rle['counts']) if text else True
            seg = {'size': [h, w], 'counts': text if text else [int(c) for c in rle['counts']]}
            forms.append(U.FORM_STRING if text else U.FORM_COUNTS), strings.append(text), polys.append([])
        gt_rle.append(rle)
        gts.append(dict(id=n + 1, image_id=a['image'] + 1, category_id=a['category'] + 1, segmentation=seg, area=float(a['area']),
                        iscrowd=int(a['iscrowd']), ignore=int(a['ignore'])))
    dts, dt_rle = [], []
    for n, d in enumerate(s['dt']):
        rle = api.encode(d['mask']) if d['mask'] is not None else gt_rle[d['of']]
        dt_rle.append(rle)
        dts.append(dict(id=n + 1, image_id=d['image'] + 1, category_id=d['category'] + 1,
                        segmentation={'size': list(rle['size']), 'counts': [int(c) for c in rle['counts']]}, score=float(d['score']),
                        area=float(api.area(rle)), bbox=[float(v) for v in api.bbox(rle)], iscrowd=0))
    E = cocoeval.COCOeval(StandIn(gts, I, K, sizes), StandIn(dts, I, K, sizes))
    E.params.useSegm = 1
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
    rank, scores, dtm, dtig, gtm, gtig, ious, iou_off = [], [], [], [], [], [], [], [0]
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
            # the whole problem's matrix in arrival order, from rleIou itself
            mat = api.iou([dt_rle[d - 1] for d in dids], [gt_rle[g - 1] for g in gids], [gts[g - 1]['iscrowd'] for g in gids])
            mat = np.asarray(mat, np.float64).reshape(len(dids), len(gids))
            ious.append(mat.reshape(-1))
            iou_off.append(iou_off[-1] + mat.size)
    cat = lambda arrs: np.concatenate(arrs, axis=-1)
    res = dict(dt_rank=cat(rank), dt_scores=cat(scores), dt_match=cat(dtm), dt_ignore=cat(dtig), gt_match=cat(gtm), gt_ignore=cat(gtig),
               precision=E.eval['precision'], recall=E.eval['recall'], stats=np.asarray(E.stats, np.float64))
    return dict(res=res, gt_rle=gt_rle, dt_rle=dt_rle, forms=forms, strings=strings, polys=polys, gts=gts, dts=dts,
                iou=np.concatenate(ious), iou_off=np.array(iou_off, np.int32), gt_of=gt_of, dt_of=dt_of)


def check(name, s, r, api):
    """the conditions that keep a test from passing idly, on the reference's own output"""
    res = r['res']
    matched = res['dt_match'][0] != 0                       # area range 'all'
    assert matched.any(axis=1).all() and (~matched).any(axis=1).all(), '%s: a threshold lacks matched or unmatched detections' % name
    gate = between = quirk = 0
    for key, dids in r['dt_of'].items():
        for d in dids:
            for g in r['gt_of'].get(key, []):
                D, G = r['dt_rle'][d - 1], r['gt_rle'][g - 1]
                if api.bb_iou(api.bbox(D), api.bbox(G)) > 0:
                    gate += 1
                    v = float(api.iou([D], [G], [r['gts'][g - 1]['iscrowd']])[0, 0])
                    between += 0 < v < 1
                elif api.area(api.merge([D, G], intersect=1)) > 0:
                    quirk += 1
    if name == 'seeded':
        above = float(np.mean(res['precision'] > -1))
        assert 0.2 <= res['stats'][0] <= 0.8, res['stats']
        assert above >= 0.9, above
        assert 2 * between >= gate > 0, (between, gate)
        assert any(a['iscrowd'] for a in s['gt']) and any(f == U.FORM_STRING for f in r['forms'])
    if name == 'hand':
        assert quirk >= 1, 'no pair with common pixels and an IoU of 0 through the column wrap'
        assert any(a['iscrowd'] for a in s['gt'])
    if name == 'edge':
        cases = {a.get('case') for a in s['gt']} | {d.get('case') for d in s['dt']}
        assert set(U.EDGE_CASES) <= cases, sorted(set(U.EDGE_CASES) - cases)
        by = {a['case']: (n, a) for n, a in enumerate(s['gt']) if a.get('case')}
        rle = lambda case: r['gt_rle'][by[case][0]]
        h0, w0 = (int(v) for v in s['sizes'][0])
        assert api.area(rle('polygon wholly outside')) == 0
        assert len(rle('polygon covering the last pixel')['counts']) % 2 == 0          # the last run is a run of ones
        assert api.bbox(rle('full image height'))[3] == h0
        assert any(len(a['seg'][1]) > 1 for a in s['gt'] if a['seg'][0] == 'poly'), 'no multi-part annotation'
        assert any(a['iscrowd'] and f == U.FORM_STRING for a, f in zip(s['gt'], r['forms']))
        assert any(a['iscrowd'] and f == U.FORM_COUNTS for a, f in zip(s['gt'], r['forms']))
        band = [5 * v + .5 for v in by['negative coordinates in the truncation band'][1]['seg'][1][0]]
        assert any(-1 < v < 0 for v in band)
        zero, one = [d for d in s['dt'] if d.get('case') == 'all-zero detection'], [d for d in s['dt'] if d.get('case') == 'all-one detection']
        assert zero[0]['mask'].sum() == 0 and one[0]['mask'].all()
    return gate, between, quirk


def main():
    assert os.path.isfile(os.path.join(PYCOCO, 'cocoeval.py')), 'the reference is not here: this script runs in the build container only'
    tmp = tempfile.mkdtemp(prefix='cocosegm_golden_')
    try:
        cocoeval, api = load_reference(tmp)
        out = {}
        for name, s in U.make_sets().items():
            r = run_reference(cocoeval, api, s)
            gate, between, quirk = check(name, s, r, api)
            res = r['res']
            print('%-6s K %d I %2d annotations %3d detections %3d kept %3d  stats[0] %.4f  precision above -1: %.3f  pairs past the box '
                  'gate %d (%d with 0 < IoU < 1), common pixels but IoU 0: %d' % (
                      name, s['K'], s['I'], len(s['gt']), len(s['dt']), len(res['dt_rank']), res['stats'][0],
                      float(np.mean(res['precision'] > -1)), gate, between, quirk))
            o = lambda k, v: out.__setitem__('%s_%s' % (name, k), v)
            o('shape', np.array([s['K'], s['I']], np.int32)), o('sizes', s['sizes'])
            for k, dtype in (('image', np.int32), ('category', np.int32), ('area', np.float64), ('iscrowd', np.int32), ('ignore', np.int32)):
                o('gt_' + k, np.array([a[k] for a in s['gt']], dtype))
            o('gt_form', np.array(r['forms'], np.int32))
            cnts, off = U.pool([g['counts'] for g in r['gt_rle']])
            o('gt_cnts', cnts), o('gt_cnt_off', off)
            sb = [np.frombuffer(t.encode('ascii'), np.uint8) for t in r['strings']]
            o('gt_str', np.concatenate(sb) if sb else np.zeros(0, np.uint8)), o('gt_str_off', np.concatenate([[0], np.cumsum([len(b) for b in sb])]).astype(np.int32))
            flat = [np.asarray(p, np.float64) for ps in r['polys'] for p in ps]
            o('poly_xy', np.concatenate(flat) if flat else np.zeros(0)), o('poly_off', np.concatenate([[0], np.cumsum([len(p) for p in flat])]).astype(np.int32))
            o('ann_poly_off', np.concatenate([[0], np.cumsum([len(ps) for ps in r['polys']])]).astype(np.int32))
            for k, dtype in (('image', np.int32), ('category', np.int32), ('score', np.float64)):
                o('dt_' + k, np.array([d[k] for d in s['dt']], dtype))
            cnts, off = U.pool([d['counts'] for d in r['dt_rle']])
            o('dt_cnts', cnts), o('dt_cnt_off', off)
            o('dt_area', np.array([d['area'] for d in r['dts']], np.float64)), o('dt_bbox', np.array([d['bbox'] for d in r['dts']], np.float64).reshape(-1, 4))
            o('iou', r['iou']), o('iou_off', r['iou_off'])
            for k in U.RESULT_KEYS:
                o('res_' + k, np.ascontiguousarray(res[k].transpose(0, 2, 3, 4, 1)) if k == 'precision' else res[k])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(U.GOLDEN, **out)
    print('wrote', U.GOLDEN, os.path.getsize(U.GOLDEN), 'bytes')


if __name__ == '__main__':
    main()
