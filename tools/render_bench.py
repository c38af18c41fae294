"""Detections drawn into a batch of synthetic images -- 480 x 640, 80 classes, --dets detections per image, every one above the
threshold, optionally with its 28 x 28 mask -- by sniper_amd.visualization, measured in its stages.

    python tools/render_bench.py [--images 64] [--dets 100] [--masks] [--out profiles/render_bench.txt]

Stages: the draw lists (host: threshold, rounding, label strings), packing them into the call's tables (host), upload (images and
tables), the kernel (sn_render_dets, the mean of --reps launches after a warm-up call), download, and the PNG encoding of every picture
(PIL).  Beside the kernel: torch's device-to-device copy of the same bytes in the same process (the floor of a pass that reads and
writes every pixel once), and the numpy restatement (tests/render_ref.py) on the first --ref-images images, whose pictures must be
equal byte for byte.  A run without items gives the cost of the pass alone; a last run confines every item to the top-left corner of its image, where
the few tiles that hold every item set the kernel's length while all other tiles pay one rect test per item."""
import argparse
import io
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, K, M = 480, 640, 80, 28


def make_problem(n_images, n_dets, with_masks, corner=False, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:M, 0:M].astype(np.float32)
    images = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n_images)]
    dets, masks = [], []
    for _ in range(n_images):
        if corner:
            bw, bh = rs.uniform(4, 40, (2, n_dets))
            x1, y1 = rs.uniform(0, 20, n_dets), rs.uniform(0, 4, n_dets)
            rows = np.stack((x1, y1, np.minimum(x1 + bw, 62), np.minimum(y1 + bh * 0.25, 14), rs.uniform(0.5, 1, n_dets)), axis=1).astype(np.float32)
        else:
            bw, bh = np.exp(rs.uniform(np.log(8), np.log(300), (2, n_dets)))
            x1, y1 = rs.uniform(0, W - 8, n_dets), rs.uniform(0, H - 8, n_dets)
            rows = np.stack((x1, y1, np.minimum(x1 + bw, W - 1), np.minimum(y1 + bh, H - 1), rs.uniform(0.5, 1, n_dets)), axis=1).astype(np.float32)
        cy, cx, ry, rx = rs.uniform(9, 19, (4, n_dets, 1, 1)).astype(np.float32)
        prob = np.clip(1.3 - ((yy - cy) / (0.8 * ry)) ** 2 - ((xx - cx) / (0.8 * rx)) ** 2, 0, 1)
        cls = rs.randint(K, size=n_dets)
        dets.append([[]] + [rows[cls == k] for k in range(K)])
        masks.append([None] + [prob[cls == k] for k in range(K)] if with_masks else None)
    return images, dets, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--masks', action='store_true')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ref-images', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'render_bench.txt'))
    a = ap.parse_args()
    import torch
    from PIL import Image
    import render_ref as ref
    from sniper_amd import visualization as V
    names = ['__background__'] + ['class%02d' % k for k in range(K)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    lim = V._limits()
    say('render: %d images of %d x %d, %d detections per image%s; tile %d x %d, %d items per culling round, %d threads; card: %s (%s, %d CUs)' % (
        a.images, H, W, a.dets, ' with %d x %d masks' % (M, M) if a.masks else '', lim['tile_w'], lim['tile_h'], lim['round'], lim['threads'],
        torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count))
    atlas = V.default_atlas()
    nbytes = a.images * H * W * 3
    # torch's copy of the same bytes
    src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(a.reps):
        dst.copy_(src)
    torch.cuda.synchronize()
    copy_s = (time.perf_counter() - t) / a.reps
    say('torch copy of the same %.1f MB (read once, written once): %.3f ms, %.0f GB/s' % (nbytes / 1e6, 1e3 * copy_s, 2 * nbytes / copy_s / 1e9))
    del src, dst
    kernel = {}
    images, _, _ = make_problem(a.images, 0, False)
    none = [V.draw_list([[]], 1.0, names) for _ in images]
    V.render_lists(images[:1], none[:1], atlas)                              # warm-up
    tm = {}
    V.render_lists(images, none, atlas, timing=tm, repeat=a.reps)
    pass_s = tm['kernel_s'] / a.reps
    say('no items at all (the pass alone: byte loads of the source, byte stores of the picture): kernel %.3f ms, %.2f x the copy' % (
        1e3 * pass_s, pass_s / copy_s))
    for corner in (False, True):
        images, dets, masks = make_problem(a.images, a.dets, a.masks, corner)
        t = time.perf_counter()
        lists = [V.draw_list(dets[i], 1.0, names, 0.5, masks[i], (H, W)) for i in range(a.images)]
        t_list = time.perf_counter() - t
        V.render_lists(images[:1], lists[:1], atlas)                         # warm-up
        tm = {}
        pics = V.render_lists(images, lists, atlas, timing=tm, repeat=a.reps)
        k_s = tm['kernel_s'] / a.reps
        kernel[corner] = k_s
        if corner:
            say('every item confined to the top-left corner of its image (a few tiles): kernel %.3f ms, %.2f x the copy' % (1e3 * k_s, k_s / copy_s))
            continue
        t = time.perf_counter()
        size = 0
        for p in pics:
            buf = io.BytesIO()
            Image.fromarray(p).save(buf, format='PNG')
            size += buf.tell()
        t_png = time.perf_counter() - t
        row = lambda what, s: say('  %-72s %9.3f ms' % (what, 1e3 * s))
        say('items spread over the images (%d items, %d glyphs of %s):' % (sum(len(l['rects']) for l in lists), sum(len(s) for l in lists for s in l['labels']),
                                                                         'no font' if atlas is None else '%d x %d' % atlas.shape[1:]))
        row('draw lists (host: threshold, rounding, label strings%s)' % (', paste boxes' if a.masks else ''), t_list)
        row('packing the tables (host)', tm['pack_s'])
        row('upload (images and tables)', tm['upload_s'])
        row('kernel sn_render_dets (mean of %d launches)' % a.reps, k_s)
        row('download', tm['download_s'])
        row('PNG encoding (PIL), %.1f MB' % (size / 1e6), t_png)
        say('kernel: %.3f ms = %.2f x the copy, %.0f GB/s of source and picture bytes; %.3f ms of it is the pass alone, %.3f ms the items' % (
            1e3 * k_s, k_s / copy_s, 2 * nbytes / k_s / 1e9, 1e3 * pass_s, 1e3 * (k_s - pass_s)))
        m = min(a.ref_images, a.images)
        t = time.perf_counter()
        same = True
        for i in range(m):
            L = dict(lists[i], text=[V.encode_text(s) for s in lists[i]['labels']])
            same &= bool(np.array_equal(ref.render(images[i], L, atlas), pics[i]))
        say('numpy restatement on the first %d images: %.2f s per image; pictures %s' % (m, (time.perf_counter() - t) / max(m, 1),
                                                                                        'equal byte for byte' if same else 'DIFFER'))
        assert same
    say('culling: the corner run costs %.2f x the spread run' % (kernel[True] / kernel[False]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
