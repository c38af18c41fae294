"""A batch of JPEG files decoded into device tensors -- 64 files of 480 x 640 (4:2:0, quality 75), and a batch of 20 -- by this
project's decoder (sniper_amd/jpeg.py: parse on the host, entropy decoding, DC scan, IDCT, upsampling and colour on the device) beside
the parent path on the same files in the same process (data.im_worker.load_bgr + upload: PIL on the host), on one thread and on
decode_ahead's 8 threads, measured in its stages.

    python tools/jpeg_bench.py [--images 64] [--out profiles/jpeg_bench.txt] [--subs 32,64,128,256,512]

Two kinds of content: seeded low-pass-filtered noise (the nearest a synthetic picture comes to a photograph) and uniform noise (the most
bits a file of this size holds).  Per kind, after a warm-up call: the stages of decode_jpeg, each closed by a synchronise; the whole call
without those synchronises; the parent path; every output compared with PIL's; the rounds the segments took; the whole call at other
subsequence sizes."""
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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_bench.txt'))
    ap.add_argument('--subs', default='32,64,128,256,512')
    a = ap.parse_args()
    import torch
    from multiprocessing.pool import ThreadPool
    from PIL import Image
    from png_bench import backgrounds
    from sniper_amd import hip, jpeg
    from sniper_amd.data.im_worker import load_bgr
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    card = '%s (%s, %d CUs)' % (torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count)
    lim = jpeg.jpeg_limits()
    say('jpeg: files of 480 x 640, 4:2:0, quality 75; subsequences of %d bytes, %d threads per segment; host CPUs in use: %s; card: %s' % (
        lim['sub'], lim['threads'], os.environ.get('OMP_NUM_THREADS', '?'), card))
    stages = (('read_s', 'file read'), ('parse_s', 'parse_jpeg (markers, tables: host)'), ('tables_s', 'pooling the bytes and tables (host)'),
              ('upload_s', 'upload (one copy) and the buffers'), ('rounds_s', 'entropy rounds + block scan (sn_jpeg_entropy, phase 1)'),
              ('write_s', 'coefficient write pass (sn_jpeg_entropy, phase 2)'), ('dc_s', 'DC scan (sn_jpeg_dc)'),
              ('pixels_s', 'IDCT + upsample + colour (sn_jpeg_pixels)'), ('status_s', 'read-back of the statuses'))
    pool = ThreadPool(8)

    def parent(paths, threads):
        t = time.perf_counter()
        if threads == 1:
            out = [hip.dev(load_bgr(p)) for p in paths]
        else:
            out = pool.map(lambda p: hip.dev(load_bgr(p)), paths, chunksize=1)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out

    with tempfile.TemporaryDirectory() as tmp:
        for kind in ('low-pass noise', 'uniform noise'):
            paths = []
            for i, im in enumerate(backgrounds(kind, a.images)):
                paths.append(os.path.join(tmp, '%s_%d.jpg' % (kind.split()[0], i)))
                Image.fromarray(im).save(paths[-1], 'JPEG', quality=75, subsampling=2)
            for n in (a.images, 20):
                batch = paths[:n]
                jpeg.decode_jpeg(batch[:2])                                  # warm-up of both paths
                parent(batch[:2], 1)
                parent(batch[:8], 8)
                jpeg.reset_stats()
                tm = {}
                jpeg.decode_jpeg(batch, timing=tm)
                torch.cuda.synchronize()
                best = None
                for _ in range(3):
                    t = time.perf_counter()
                    got = jpeg.decode_jpeg(batch)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t
                    best = dt if best is None else min(best, dt)
                one_s, want = parent(batch, 1)
                one_s = min(one_s, parent(batch, 1)[0])
                eight_s = min(parent(batch, 8)[0], parent(batch, 8)[0])
                same = all(torch.equal(g, w) for g, w in zip(got, want))
                st = jpeg.stats()
                rounds = np.array(tm['rounds'])
                say('%s, %d files, %.2f MB compressed for %.2f MB of pixels, card: %s' % (kind, n, sum(os.path.getsize(p) for p in batch) / 1e6,
                                                                                        n * 480 * 640 * 3 / 1e6, card))
                host_s = 0.0
                for key, what in stages:
                    say('  %-72s %9.3f ms   [%s]' % (what, 1e3 * tm.get(key, 0.0), card))
                    if key in ('read_s', 'parse_s', 'tables_s'):
                        host_s += tm.get(key, 0.0)
                say('  %-72s %9.3f ms   [%s]' % ('decode_jpeg, the whole call (no synchronise between the stages), best of 3', 1e3 * best, card))
                say('  %-72s %9.3f ms   [%s]' % ('parent path: load_bgr + upload, one host thread, best of 2', 1e3 * one_s, card))
                say('  %-72s %9.3f ms   [%s]' % ('parent path: load_bgr + upload on decode_ahead\'s 8 threads, best of 2', 1e3 * eight_s, card))
                say('  decode_jpeg is %.2f x as fast as one thread and %.2f x as fast as 8 threads; host stages %.3f ms of the call; rounds per segment: '
                    'min %d, median %d, max %d; decoded on the device: %d of %d; every output %s PIL\'s   [%s]' % (
                        one_s / best, eight_s / best, 1e3 * host_s, rounds.min(), int(np.median(rounds)), rounds.max(),
                        st['device'] // 4, n, 'equals' if same else 'DIFFERS FROM', card))
                assert same
                if n == a.images:
                    for sub in [int(v) for v in a.subs.split(',') if v]:
                        tm2 = {}
                        jpeg.decode_jpeg(batch, timing=tm2, sub=sub)
                        t = time.perf_counter()
                        jpeg.decode_jpeg(batch, sub=sub)
                        torch.cuda.synchronize()
                        dt = time.perf_counter() - t
                        r2 = np.array(tm2['rounds'])
                        say('  subsequences of %4d bytes: rounds %8.3f ms, write pass %8.3f ms, whole call %8.3f ms, rounds per segment median %d, max %d   [%s]' % (
                            sub, 1e3 * tm2['rounds_s'], 1e3 * tm2['write_s'], 1e3 * dt, int(np.median(r2)), r2.max(), card))
                del got, want
    pool.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
