"""A batch of PNG files decoded into device tensors -- 64 files of 480 x 640 RGB -- by this project's decoder (sniper_amd/png_decode.py:
chunk walk and CRC-32 on the host, inflate, unfilter and expansion on the device) beside the parent path on the same files in the same
process (data.im_worker.load_bgr + upload: PIL on the host), on one thread and on decode_ahead's 8 threads, measured in its stages.

    python tools/png_dec_bench.py [--images 64] [--dets 100] [--out profiles/png_dec_bench.txt]

Four groups of files: PIL-saved low-pass noise (the nearest a synthetic picture comes to a photograph), PIL-saved uniform noise (the most
bits a file of this size holds), PIL-saved pictures of one colour, and a rendered batch (detections drawn into low-pass noise) written
by this project's own write_png (run matches at distance 1, one distance code, empty stored blocks).  Per group, after a warm-up
call: the stages of decode_png, each closed by a synchronise; the whole call without those synchronises; the parent path; every output
compared with PIL's."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'png_dec_bench.txt'))
    a = ap.parse_args()
    import torch
    from multiprocessing.pool import ThreadPool
    from PIL import Image
    from png_bench import H, W, backgrounds
    from render_bench import K, make_problem
    from sniper_amd import hip, png, png_decode
    from sniper_amd import visualization as V
    from sniper_amd.data.im_worker import load_bgr
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    card = '%s (%s, %d CUs)' % (torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count)
    lim = png_decode.inflate_limits()
    say('png decode: %d files of %d x %d RGB; one wave of %d lanes per stream, %d bytes of LDS per wave; host CPUs in use: %s; card: %s' % (
        a.images, H, W, lim['lanes'], lim['lds'], os.environ.get('OMP_NUM_THREADS', '?'), card))
    stages = (('read_s', 'file read'), ('parse_s', 'parse_png (chunks, CRC-32: host)'), ('tables_s', 'pooling the bytes and tables (host)'),
              ('upload_s', 'upload (one copy) and the buffers'), ('inflate_s', 'inflate (sn_inflate)'), ('unfilter_s', 'unfilter (sn_png_unfilter)'),
              ('expand_s', 'expansion to BGR (sn_png_expand)'), ('status_s', 'read-back of the lengths and statuses'))
    pool = ThreadPool(8)

    def parent(paths, threads):
        t = time.perf_counter()
        if threads == 1:
            out = [hip.dev(load_bgr(p)) for p in paths]
        else:
            out = pool.map(lambda p: hip.dev(load_bgr(p)), paths, chunksize=1)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    names = ['__background__'] + ['class%02d' % k for k in range(K)]
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ('low-pass noise', 'uniform noise', 'one colour', 'rendered, written by write_png'):
            paths = [os.path.join(tmp, '%s_%d.png' % (kind.split()[0].strip(','), i)) for i in range(a.images)]
            if kind.startswith('rendered'):
                _, dets, _ = make_problem(a.images, a.dets, False)
                lists = [V.draw_list(dets[i], 1.0, names, 0.5, None, (H, W)) for i in range(a.images)]
                images = [torch.as_tensor(im).cuda() for im in backgrounds('low-pass noise', a.images)]
                png.write_png(paths, V.render_lists(images, lists, V.default_atlas()))
            else:
                for p, im in zip(paths, backgrounds(kind, a.images)):
                    Image.fromarray(im).save(p, 'PNG')
            png_decode.decode_png(paths[:2])                                  # warm-up of both paths
            parent(paths[:2], 1)
            parent(paths[:8], 8)
            png_decode.reset_stats()
            tm = {}
            png_decode.decode_png(paths, timing=tm)
            torch.cuda.synchronize()
            best = None
            for _ in range(3):
                t = time.perf_counter()
                got = png_decode.decode_png(paths)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                best = dt if best is None else min(best, dt)
            one_s, want = parent(paths, 1)
            one_s = min(one_s, parent(paths, 1)[0])
            eight_s = min(parent(paths, 8)[0], parent(paths, 8)[0])
            same = all(torch.equal(g, w) for g, w in zip(got, want))
            st = png_decode.stats()
            say('%s, %d files, %.2f MB compressed for %.2f MB of pixels, card: %s' % (kind, a.images, sum(os.path.getsize(p) for p in paths) / 1e6,
                                                                                    a.images * H * W * 3 / 1e6, card))
            host_s = 0.0
            for key, what in stages:
                say('  %-72s %9.3f ms   [%s]' % (what, 1e3 * tm.get(key, 0.0), card))
                if key in ('read_s', 'parse_s', 'tables_s'):
                    host_s += tm.get(key, 0.0)
            say('  %-72s %9.3f ms   [%s]' % ('decode_png, the whole call (no synchronise between the stages), best of 3', 1e3 * best, card))
            say('  %-72s %9.3f ms   [%s]' % ('parent path: load_bgr + upload, one host thread, best of 2', 1e3 * one_s, card))
            say('  %-72s %9.3f ms   [%s]' % ('parent path: load_bgr + upload on decode_ahead\'s 8 threads, best of 2', 1e3 * eight_s, card))
            say('  decode_png is %.2f x as fast as one thread and %.2f x as fast as 8 threads; host stages %.3f ms of the call; decoded on the '
                'device: %d of %d, fallbacks %s; every output %s PIL\'s   [%s]' % (
                    one_s / best, eight_s / best, 1e3 * host_s, st['device'] // 4, a.images, st['fallback'] or 'none',
                    'equals' if same else 'DIFFERS FROM', card))
            assert same
            del got, want
    pool.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
