"""A rendered batch written as PNG files -- 64 pictures of 480 x 640 with 100 detections each -- by this project's encoder
(sniper_amd/png.py: filters and deflate on the device, container and CRC-32 on the host) beside the parent path on the same pictures in
the same process (visualization._save: download, then PIL on one host thread), measured in its stages.

    python tools/png_bench.py [--images 64] [--dets 100] [--out profiles/png_bench.txt]

Three kinds of background: seeded low-pass-filtered noise (the nearest a synthetic picture comes to a photograph: smooth, with
sensor-like noise on top), uniform noise (what tools/render_bench.py renders onto: incompressible) and one colour.  Per kind, after a
warm-up call: the stages of write_png, each closed by a synchronise; the whole call without those synchronises; the parent path; the
file sizes of both; and the first pictures of both decoded and compared."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

H, W = 480, 640


def _box(a, r, axis):
    """box filter of radius r along an axis, edges repeated"""
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r + 1, r)
    c = np.cumsum(np.pad(a, pad, mode='edge'), axis=axis, dtype=np.float64)
    n = a.shape[axis]
    hi = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis)
    lo = np.take(c, np.arange(0, n), axis=axis)
    return (hi - lo) / (2 * r + 1)


def backgrounds(kind, n, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        if kind == 'low-pass noise':
            x = rs.uniform(0, 1, (H, W, 3))
            for _ in range(2):
                x = _box(_box(x, 12, 0), 12, 1)
            x = (x - x.min()) / max(x.max() - x.min(), 1e-9)
            x = 255 * x + rs.normal(0, 2.0, (H, W, 3))               # sensor-like noise of two levels
            out.append(np.clip(np.rint(x), 0, 255).astype(np.uint8))
        elif kind == 'uniform noise':
            out.append(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
        else:
            out.append(np.tile(rs.randint(0, 256, (1, 1, 3)).astype(np.uint8), (H, W, 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_bench.txt'))
    a = ap.parse_args()
    import torch
    from PIL import Image
    from render_bench import K, make_problem
    from sniper_amd import png
    from sniper_amd import visualization as V
    names = ['__background__'] + ['class%02d' % k for k in range(K)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    card = '%s (%s, %d CUs)' % (torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count)
    lim = png.deflate_limits()
    say('png: %d pictures of %d x %d, %d detections drawn into each; deflate blocks of %d bytes, %d threads; card: %s' % (
        a.images, H, W, a.dets, lim['block'], lim['threads'], card))
    _, dets, _ = make_problem(a.images, a.dets, False)
    lists = [V.draw_list(dets[i], 1.0, names, 0.5, None, (H, W)) for i in range(a.images)]
    atlas = V.default_atlas()
    stages = (('upload_s', 'pictures to one buffer (device copy) and the tables'), ('filter_s', 'filter kernel (sn_png_filter)'),
              ('code_s', 'plan + histogram / code kernel (sn_deflate_code)'), ('scan_s', 'scan of the block sizes (torch.cumsum)'),
              ('write_s', 'write kernel (sn_deflate_write)'), ('lengths_s', 'read-back of the stream lengths'),
              ('download_s', 'download of the compressed bytes'), ('container_s', 'CRC-32 and container (host, zlib.crc32)'),
              ('file_s', 'file writes'))
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ('low-pass noise', 'uniform noise', 'one colour'):
            images = [torch.as_tensor(im).cuda() for im in backgrounds(kind, a.images)]
            pics = V.render_lists(images, lists, atlas)                      # device tensors: the rendered batch where it lies
            torch.cuda.synchronize()
            dev_paths = [os.path.join(tmp, 'dev_%d.png' % i) for i in range(a.images)]
            pil_paths = [os.path.join(tmp, 'pil_%d.png' % i) for i in range(a.images)]
            png.write_png(dev_paths[:2], pics[:2])                           # warm-up of both paths
            V._save(pics[0].cpu().numpy(), pil_paths[0])
            tm = {}
            png.write_png(dev_paths, pics, timing=tm)
            torch.cuda.synchronize()
            t = time.perf_counter()
            png.write_png(dev_paths, pics)
            dev_s = time.perf_counter() - t
            t = time.perf_counter()
            for p, path in zip(pics, pil_paths):                             # the parent path: visualization._save of every picture
                V._save(p.cpu().numpy(), path)
            pil_s = time.perf_counter() - t
            dev_b = sum(os.path.getsize(p) for p in dev_paths)
            pil_b = sum(os.path.getsize(p) for p in pil_paths)
            same = all(np.array_equal(np.asarray(Image.open(dev_paths[i])), np.asarray(Image.open(pil_paths[i]))) for i in range(min(4, a.images)))
            say('%s, card: %s' % (kind, card))
            for key, what in stages:
                say('  %-72s %9.3f ms   [%s]' % (what, 1e3 * tm.get(key, 0.0), card))
            say('  %-72s %9.3f ms   [%s]' % ('write_png, the whole call (no synchronise between the stages)', 1e3 * dev_s, card))
            say('  %-72s %9.3f ms   [%s]' % ('parent path: download + PIL save of every picture (one host thread)', 1e3 * pil_s, card))
            say('  write_png is %.2f x as fast as the parent path; files %.2f MB against PIL\'s %.2f MB (%.3f x); first pictures decode %s   [%s]' % (
                pil_s / dev_s, dev_b / 1e6, pil_b / 1e6, dev_b / max(pil_b, 1), 'equal' if same else 'DIFFERENT', card))
            assert same
            del images, pics
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
