"""The results file of one val-sized synthetic mask problem -- 5 000 images of 480 x 640, 80 classes, 100 detections per image, every
mask a 28 x 28 probability map in its box -- written and read back (sniper_amd.results), measured in its stages, beside the host
coders on the same node.

    python tools/coco_results_bench.py [--images 5000] [--dets 100] [--ref-images 0] [--out profiles/coco_results_bench.txt]

write_coco_results(..., 'segm'): paste (rle_paste: upload of the maps, sn_rle_paste_count, the read-back, sn_rle_paste, download of
the counts), the string coder (upload of the pooled counts, sn_rle_string_len, the read-back, sn_rle_to_string), the download of the
characters, the assembly of the records (Python: cells, boxes, dicts, slicing the strings) and json.dump.  load_coco_results: json.load,
the records' ids and sizes (Python), the string decoder (upload, sn_rle_string_count, the read-back, sn_rle_from_string), the download
of the counts, the bounding boxes (sn_rle_stats) and the cells.  Every stage is closed by a synchronise; one run after a small
warm-up call (the problem is too large to repeat for medians within a short job).
The host coders -- evaluation.rle_from_string, the per-character loop, and a plain-Python rleToString (tests/rle_string_ref.py) -- run
on the records of the first --ref-images images (0 = all; their cost is linear in the characters) and on those the strings and the
counts must be equal byte for byte."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, K, M = 480, 640, 80, 28


def make_problem(n_images, n_dets, seed=0):
    """per image n_dets detections of random classes: a box of 8 .. 300 pixels a side, a smooth blob of probabilities in it"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:M, 0:M].astype(np.float32)
    boxes = [[np.zeros((0, 5), np.float32) for _ in range(n_images)] for _ in range(K + 1)]
    masks = [[np.zeros((0, M, M), np.float32) for _ in range(n_images)] for _ in range(K + 1)]
    for i in range(n_images):
        bw, bh = np.exp(rs.uniform(np.log(8), np.log(300), (2, n_dets)))
        x1, y1 = rs.uniform(0, W - 8, n_dets), rs.uniform(0, H - 8, n_dets)
        rows = np.stack((x1, y1, np.minimum(x1 + bw, W - 1), np.minimum(y1 + bh, H - 1), rs.uniform(0.001, 1, n_dets)), axis=1).astype(np.float32)
        cy, cx, ry, rx = rs.uniform(9, 19, (4, n_dets, 1, 1)).astype(np.float32)
        prob = np.clip(1.3 - ((yy - cy) / (0.8 * ry)) ** 2 - ((xx - cx) / (0.8 * rx)) ** 2, 0, 1)
        cls = rs.randint(K, size=n_dets)
        for k in np.unique(cls):
            sel = cls == k
            boxes[k + 1][i], masks[k + 1][i] = rows[sel], prob[sel]
    return boxes, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--ref-images', type=int, default=0, help='0 = all')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'coco_results_bench.txt'))
    a = ap.parse_args()
    import torch
    import rle_string_ref as ref
    from sniper_amd.evaluation import rle_from_string
    from sniper_amd.results import load_coco_results, write_coco_results
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    say('COCO segm results file, %d images of %d x %d x %d classes x %d detections per image, %d x %d probability maps as input; card: %s (%s, %d CUs)' % (
        a.images, H, W, K, a.dets, M, M, torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    t = time.perf_counter()
    boxes, masks = make_problem(a.images, a.dets)
    say('problem made in %.1f s' % (time.perf_counter() - t))
    image_ids, cat_ids, sizes = list(range(1, a.images + 1)), list(range(1, K + 1)), np.tile([[H, W]], (a.images, 1))
    tmp = tempfile.mkdtemp(prefix='coco_results_bench_')
    path = os.path.join(tmp, 'detections_val_results.json')
    try:
        write_coco_results(path, [per[:2] for per in boxes], image_ids[:2], cat_ids, 'segm', [per[:2] for per in masks], sizes[:2])      # warm-up
        tw = {}
        t = time.perf_counter()
        n = write_coco_results(path, boxes, image_ids, cat_ids, 'segm', masks, sizes, timing=tw)
        torch.cuda.synchronize()
        total_w = time.perf_counter() - t
        nbytes = os.path.getsize(path)
        rest = total_w - tw['paste_s'] - tw['encode_s'] - tw['encode_download_s'] - tw['json_dump_s']
        say('%d records, %d counts (%.0f per mask), %d characters (%.2f per count), file of %.1f MB' % (
            n, tw['runs'], tw['runs'] / n, tw['chars'], tw['chars'] / tw['runs'], nbytes / 1e6))
        row = lambda what, s, total: say('  %-86s %9.1f ms  %5.1f %%' % (what, 1e3 * s, 100 * s / total))
        say('write_coco_results(segm): %.1f ms' % (1e3 * total_w))
        row('paste: rle_paste (upload of the maps, sn_rle_paste_count, read-back, sn_rle_paste, download)', tw['paste_s'], total_w)
        row('string coder: upload of the counts, sn_rle_string_len, read-back, sn_rle_to_string', tw['encode_s'], total_w)
        row('download of the characters and decoding them to one str', tw['encode_download_s'], total_w)
        row('record assembly (Python: cells, paste_boxes, dicts, slicing the strings)', rest, total_w)
        row('json.dump(sort_keys=True, indent=4)', tw['json_dump_s'], total_w)
        t = time.perf_counter()
        with open(path) as fh:
            recs = json.load(fh)
        t_json = time.perf_counter() - t
        tl = {}
        t = time.perf_counter()
        got_boxes, got_masks = load_coco_results(recs, image_ids, cat_ids, sizes, timing=tl)
        torch.cuda.synchronize()
        t_load = time.perf_counter() - t
        total_l = t_json + t_load
        say('load_coco_results: %.1f ms, %d strings, %d host fall-backs' % (1e3 * total_l, tl['strings'], tl['host_fallback']))
        row('json.load', t_json, total_l)
        row('string decoder: upload of the characters, sn_rle_string_count, read-back, sn_rle_from_string', tl['decode_s'], total_l)
        row('download of the counts', tl['decode_download_s'], total_l)
        row('bounding boxes: pool, upload, sn_rle_stats, download', tl['bbox_s'], total_l)
        row('records and cells (Python: ids, sizes, the order, lists of dicts)', t_load - tl['decode_s'] - tl['decode_download_s'] - tl['bbox_s'], total_l)
    finally:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    # ---- the host coders on the first images ----
    m = min(a.ref_images, a.images) if a.ref_images > 0 else a.images
    counts = [c['counts'] for k in range(1, K + 1) for i in range(m) for c in got_masks[k][i]]
    by_cell = {}
    for r in recs:
        if r['image_id'] <= m:
            by_cell.setdefault((r['category_id'], r['image_id']), []).append(r['segmentation']['counts'])
    strings = [s for k in range(1, K + 1) for i in range(1, m + 1) for s in by_cell.get((k, i), [])]
    assert len(strings) == len(counts)
    t = time.perf_counter()
    want_c = [rle_from_string(s) for s in strings]
    t_from = time.perf_counter() - t
    t = time.perf_counter()
    want_s = [ref.to_string(c) for c in counts]
    t_to = time.perf_counter() - t
    same = all(np.array_equal(g, w_) for g, w_ in zip(counts, want_c)) and want_s == strings
    scale = len(recs) / max(len(strings), 1)
    say('host coders on the %d records of %s %d images: rle_from_string (per-character loop) %.2f s, plain-Python rleToString %.2f s%s; '
        'strings and counts %s' % (len(strings), 'all' if m == a.images else 'the first', m, t_from, t_to,
                                   '' if m == a.images else ' (linear in the characters: about %.0f s and %.0f s for all %d)' % (
                                       t_from * scale, t_to * scale, len(recs)),
                                   'equal byte for byte' if same else 'DIFFER'))
    assert same
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
