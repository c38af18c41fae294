"""Generate tests/golden/proproidb_v1.npz from the REFERENCE's own lib/dataset/imdb.py (build container only; the GPU box and the
test suite read the committed file).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_proproidb_golden.py

How the reference is run (nothing translated is kept: it all lives in a temporary directory outside the repository):
  * lib/dataset/imdb.py and lib/nms/nms.py (Python 2) are copied there and lib2to3 is run on the copies;
  * the one mechanical fix a current numpy needs is applied to the copy of imdb.py: `np.float)` -> `float)`;
  * `bbox.bbox_transform` is a stub that hands out bbox_overlaps_cython of the reference's own extension, which oracle.build compiles
    into oracle/_ref/ from lib/bbox/bbox.pyx where it lies (the alias `np.float` exists while the extension initialises, as in
    oracle/ref_py.py, and not afterwards); the compiled NMS modules nms.py imports (not used by nmsp) are stubs;
  * per set: the proposals go into <name>_rpn.pkl, then IMDB.load_rpn_data (nmsp over a Pool), create_roidb_from_box_list,
    merge_roidbs into the set's ground-truth roidb, and evaluate_recall on the merged roidb, without and with candidate_boxes.

What the file holds, per set s in (small, edges, coco_like) -- arrays only: the inputs (tests/prop_roidb_util.py save_set) and
  s_keep_idx, s_keep_counts    the rows load_rpn_data returned, as indices into the image's input rows (scores are distinct, and the
                               returned rows are checked to be exactly those rows)
  s_max_overlaps, s_max_classes  of create_roidb_from_box_list's records, concatenated (gt_overlaps is checked to hold exactly
                               max_overlaps at max_classes and zeros elsewhere, and is not stored)
  s_merged_rows, s_merged_scores  per image the lengths of boxes and proposal_scores after merge_roidbs
  s_summary, s_summary_cand    evaluate_recall's string as bytes.

Conditions asserted, so that a test cannot pass without testing anything: scores distinct within every image; in coco_like the NMS
removes between 10 % and 90 % of the rows, the recall at 0.5 for `all` lies in [0.2, 0.95] and num_pos > 0 for at least five of the
seven ranges; the cases the edges set is made of (see check_edges)."""
import contextlib
import importlib.util
import io
import glob
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

import prop_roidb_ref as R  # noqa: E402
import prop_roidb_util as U  # noqa: E402
from oracle import build  # noqa: E402

BBOX_STUB = '''
import importlib.util
import numpy as np
_spec = importlib.util.spec_from_file_location('bbox', %r)
_ext = importlib.util.module_from_spec(_spec)
_alias = not hasattr(np, 'float')
if _alias:
    np.float = float      # bbox.pyx:14 spells its dtype with the alias numpy dropped; only while the extension initialises
_spec.loader.exec_module(_ext)
if _alias:
    del np.float
bbox_overlaps = _ext.bbox_overlaps_cython
ignore_overlaps = _ext.bbox_overlaps_ignore_cython if hasattr(_ext, 'bbox_overlaps_ignore_cython') else None
'''
NMS_EXT_STUB = '''
def cpu_nms(*args):
    raise NotImplementedError('compiled NMS is not part of the proposal roidb goldens')
cpu_soft_nms = gpu_nms = cpu_nms
'''


def load_reference(tmp):
    build.build_reference()
    ext = glob.glob(os.path.join(build.REF_OUT, 'bbox*.so'))
    assert len(ext) == 1, ext
    lib = os.path.join(build.REF, 'lib')
    for pkg, name in (('dataset', 'imdb.py'), ('nms', 'nms.py')):
        os.makedirs(os.path.join(tmp, pkg), exist_ok=True)
        open(os.path.join(tmp, pkg, '__init__.py'), 'w').close()
        shutil.copy(os.path.join(lib, pkg, name), os.path.join(tmp, pkg, name))
        subprocess.check_call([sys.executable, '-m', 'lib2to3', '-w', '-n', os.path.join(tmp, pkg, name)], stdout=subprocess.DEVNULL,
                              stderr=subprocess.DEVNULL)
    src = os.path.join(tmp, 'dataset', 'imdb.py')
    with open(src) as fh:
        text = fh.read()
    assert text.count('np.float)') == 4
    with open(src, 'w') as fh:
        fh.write(text.replace('np.float)', 'float)'))
    os.mkdir(os.path.join(tmp, 'bbox'))
    open(os.path.join(tmp, 'bbox', '__init__.py'), 'w').close()
    with open(os.path.join(tmp, 'bbox', 'bbox_transform.py'), 'w') as fh:
        fh.write(BBOX_STUB % ext[0])
    for where in (tmp, os.path.join(tmp, 'nms')):
        for mod in ('cpu_nms', 'gpu_nms'):
            with open(os.path.join(where, mod + '.py'), 'w') as fh:
                fh.write(NMS_EXT_STUB)
    sys.path.insert(0, tmp)
    sys.dont_write_bytecode = True
    from dataset import imdb
    return imdb


def run_reference(ref, root, name, s):
    os.makedirs(root)
    db = ref.IMDB('golden', name, root, root)
    db.num_classes, db.num_images = s['num_classes'], len(s['props'])
    for p in s['props']:
        assert len(np.unique(p[:, 4])) == len(p), 'equal scores in an image'
    with open(os.path.join(root, db.name + '_rpn.pkl'), 'wb') as fh:
        pickle.dump([p.copy() for p in s['props']], fh, pickle.HIGHEST_PROTOCOL)
    gt_roidb = U.gt_roidb_of(s)
    with contextlib.redirect_stdout(io.StringIO()), np.errstate(divide='ignore', invalid='ignore'):
        boxes, maps = db.load_rpn_data(root)
        assert maps == [] and os.path.isfile(os.path.join(root, db.name + '_rpn_after_nms.pkl'))
        rpn = db.create_roidb_from_box_list(boxes, maps, gt_roidb)
        keep_idx = []
        for p, b, rec in zip(s['props'], boxes, rpn):
            idx = np.array([int(np.flatnonzero(p[:, 4] == sc)[0]) for sc in b[:, 4]], np.int32)
            assert b.dtype == np.float32 and b.tobytes() == p[idx].tobytes()
            keep_idx.append(idx)
            dense = np.zeros_like(rec['gt_overlaps'])
            dense[np.arange(len(dense)), rec['max_classes']] = rec['max_overlaps']
            assert rec['gt_overlaps'].dtype == np.float32 and rec['gt_overlaps'].tobytes() == dense.tobytes()
        max_overlaps = np.concatenate([rec['max_overlaps'] for rec in rpn] + [np.zeros(0, np.float32)])
        max_classes = np.concatenate([rec['max_classes'] for rec in rpn] + [np.zeros(0, np.int64)])
        merged = ref.IMDB.merge_roidbs(gt_roidb, rpn)
        summary = db.evaluate_recall(merged)
        summary_cand = db.evaluate_recall(merged, candidate_boxes=boxes)
    return {'keep_idx': np.concatenate(keep_idx + [np.zeros(0, np.int32)]), 'keep_counts': np.array([len(k) for k in keep_idx], np.int32),
            'max_overlaps': max_overlaps, 'max_classes': max_classes,
            'merged_rows': np.array([len(r['boxes']) for r in merged], np.int32),
            'merged_scores': np.array([len(r['proposal_scores']) for r in merged], np.int32),
            'summary': np.frombuffer(summary.encode(), np.uint8), 'summary_cand': np.frombuffer(summary_cand.encode(), np.uint8)}, merged


def check_edges(s, res):
    keep = np.split(res['keep_idx'], np.cumsum(res['keep_counts'])[:-1])
    mo = np.split(res['max_overlaps'], np.cumsum(res['keep_counts'])[:-1])
    n, g = [len(p) for p in s['props']], [len(b) for b in s['gt_boxes']]
    assert n[0] == 0 and g[0] > 0 and g[1] == 0 and n[1] > 0 and 0 < n[2] < g[2]
    assert (mo[1] == 0).all() and mo[3][list(keep[3]).index(0)] == 0 and (mo[3] > 0).any()      # no row at all / a box that meets none
    ov = R.bbox_overlaps(s['props'][4][:, :4], s['gt_boxes'][4])
    assert ov[0, 0] == ov[0, 1] > 0                                         # two rows, one best overlap
    ov = R.bbox_overlaps(s['props'][5][:, :4], s['gt_boxes'][5])
    assert ov[0, 0] == ov[1, 0] > 0                                         # two boxes, equal overlap on one row
    a, b = s['props'][6][0], s['props'][6][1]
    inter = np.float32(10 * 7)
    assert inter / (np.float32(100) + np.float32(70) - inter) == np.float32(0.7) and sorted(keep[6]) == [0, 1]     # IoU 7 / 10 survives
    assert a[4] > b[4]
    assert R.bbox_overlaps(s['props'][7][:, :4], s['gt_boxes'][7])[0, 0] == 0.5
    gb = s['gt_boxes'][8][0]
    assert (gb[2] - gb[0] + 1) * (gb[3] - gb[1] + 1) == 25 ** 2


def main():
    assert build.have_reference(), 'the reference is not here: this script runs in the build container only'
    tmp = tempfile.mkdtemp(prefix='proproidb_golden_')
    try:
        ref = load_reference(tmp)
        out = {}
        for name, s in U.make_sets().items():
            res, merged = run_reference(ref, os.path.join(tmp, name), name, s)
            total, kept = sum(len(p) for p in s['props']), int(res['keep_counts'].sum())
            mine = R.evaluate_recall(merged)
            assert mine['summary'] == res['summary'].tobytes().decode(), 'the restatement and the reference print different strings'
            rec_all = [mine['ar'][0]] + list(mine['recalls'][0])     # (the restatement's: its string is the reference's)
            print('%-9s images %2d rows %3d proposals %5d kept %5d  recall@0.5 (all) %.3f  num_pos %s' % (
                name, len(s['props']), sum(len(b) for b in s['gt_boxes']), total, kept, rec_all[1], list(mine['num_pos'])))
            if name == 'coco_like':
                assert 0.1 <= 1 - kept / float(total) <= 0.9, (kept, total)
                assert 0.2 <= rec_all[1] <= 0.95, rec_all
                assert (mine['num_pos'] > 0).sum() >= 5, mine['num_pos']
            if name == 'edges':
                check_edges(s, res)
                assert mine['hits'][0, 0] > mine['hits'][0, 1]                  # the IoU 0.5 pair counts at 0.5 only
            U.save_set(out, name, s)
            for k in U.GOLDEN_KEYS:
                out['%s_%s' % (name, k)] = res[k]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(U.GOLDEN, **out)
    print('wrote', U.GOLDEN, os.path.getsize(U.GOLDEN), 'bytes')
    assert os.path.getsize(U.GOLDEN) <= 316525, 'larger than the largest golden file so far'


if __name__ == '__main__':
    main()
