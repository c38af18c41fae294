"""A rendered batch written as .jpg files -- 64 pictures of 480 x 640 with 100 detections each -- by this project's encoder
(sniper_amd/jpeg_encode.py: everything up to the stuffed scan on the device, headers and joining on the host), measured in its stages,
beside, in the same process on the same pictures, the parent path (visualization._save: download, then PIL on one host thread) and
write_png on the device (sniper_amd/png.py).

    python tools/jpeg_enc_bench.py [--images 64] [--dets 100] [--out profiles/jpeg_enc_bench.txt]

Three kinds of background, those of tools/png_bench.py: low-pass-filtered noise, uniform noise and one colour.  Per kind, after a
warm-up call: the stages of write_jpeg, each closed by a synchronise; the whole call without those synchronises; the parent path;
write_png; the file sizes of all three; and EVERY device file compared with PIL's, byte for byte."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--dets', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'jpeg_enc_bench.txt'))
    a = ap.parse_args()
    import torch
    from png_bench import H, W, backgrounds
    from render_bench import K, make_problem
    from sniper_amd import jpeg_encode, png
    from sniper_amd import visualization as V
    names = ['__background__'] + ['class%02d' % k for k in range(K)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    prop = torch.cuda.get_device_properties(0)
    card = '%s (%s, %d CUs)' % (torch.cuda.get_device_name(0), getattr(prop, 'gcnArchName', '?'), prop.multi_processor_count)
    lim = jpeg_encode.jpeg_enc_limits()
    say('jpeg: %d pictures of %d x %d, %d detections drawn into each; quality 75, 4:2:0; %d threads, chunks of %d bytes, %d bytes of raw '
        'capacity per block; card: %s' % (a.images, H, W, a.dets, lim['threads'], lim['chunk'], lim['raw_bytes_per_block'], card))
    _, dets, _ = make_problem(a.images, a.dets, False)
    lists = [V.draw_list(dets[i], 1.0, names, 0.5, None, (H, W)) for i in range(a.images)]
    atlas = V.default_atlas()
    stages = (('upload_s', 'pictures to one buffer (device copy) and the tables'), ('blocks_s', 'blocks kernel: colour, downsample, DCT, quantise'),
              ('size_s', 'size kernel (sn_jpeg_enc_size)'), ('scan_s', 'scans of the sizes, zeroing the raw streams (torch)'),
              ('write_s', 'write kernel (sn_jpeg_enc_write)'), ('alloc_s', 'allocating the counts and the output at its bound (torch.empty)'),
              ('count_s', 'stuffing, phase 1: bytes per chunk (sn_jpeg_enc_stuff)'), ('stuff_scan_s', 'scan of the chunk sizes (torch.cumsum)'),
              ('stuff_s', 'stuffing, phase 2: the bytes (sn_jpeg_enc_stuff), the scan offsets'),
              ('lengths_s', 'read-back of the scan lengths'), ('download_s', 'download of the compressed bytes'),
              ('join_s', 'headers and joining (host)'), ('file_s', 'file writes'))

    def read(path):
        with open(path, 'rb') as fh:
            return fh.read()
    with tempfile.TemporaryDirectory() as tmp:
        for kind in ('low-pass noise', 'uniform noise', 'one colour'):
            images = [torch.as_tensor(im).cuda() for im in backgrounds(kind, a.images)]
            pics = V.render_lists(images, lists, atlas)                      # device tensors: the rendered batch where it lies
            torch.cuda.synchronize()
            dev_paths = [os.path.join(tmp, 'dev_%d.jpg' % i) for i in range(a.images)]
            pil_paths = [os.path.join(tmp, 'pil_%d.jpg' % i) for i in range(a.images)]
            png_paths = [os.path.join(tmp, 'dev_%d.png' % i) for i in range(a.images)]
            jpeg_encode.write_jpeg(dev_paths, pics)                          # warm-up of the three paths (the encoder at its full size:
                                                                             # the allocator then holds the buffers of the timed calls)
            V._save(pics[0].cpu().numpy(), pil_paths[0])
            png.write_png(png_paths[:2], pics[:2])
            tm = {}
            jpeg_encode.write_jpeg(dev_paths, pics, timing=tm)
            torch.cuda.synchronize()
            t = time.perf_counter()
            jpeg_encode.write_jpeg(dev_paths, pics)
            dev_s = time.perf_counter() - t
            t = time.perf_counter()
            for p, path in zip(pics, pil_paths):                             # the parent path: visualization._save of every picture
                V._save(p.cpu().numpy(), path)
            pil_s = time.perf_counter() - t
            torch.cuda.synchronize()
            t = time.perf_counter()
            png.write_png(png_paths, pics)
            png_s = time.perf_counter() - t
            dev_b, pil_b, png_b = (sum(os.path.getsize(p) for p in paths) for paths in (dev_paths, pil_paths, png_paths))
            same = sum(read(d) == read(p) for d, p in zip(dev_paths, pil_paths))
            say('%s, card: %s' % (kind, card))
            for key, what in stages:
                say('  %-72s %9.3f ms   [%s]' % (what, 1e3 * tm.get(key, 0.0), card))
            say('  %-72s %9.3f ms   [%s]' % ('write_jpeg, the whole call (no synchronise between the stages)', 1e3 * dev_s, card))
            say('  %-72s %9.3f ms   [%s]' % ('parent path: download + PIL save of every picture (one host thread)', 1e3 * pil_s, card))
            say('  %-72s %9.3f ms   [%s]' % ('write_png on the device, the same pictures', 1e3 * png_s, card))
            say('  write_jpeg is %.2f x as fast as the parent path and %.2f x as fast as write_png; files %.2f MB, PIL\'s .jpg %.2f MB, device .png '
                '%.2f MB; %d of %d files equal PIL\'s byte for byte   [%s]' % (pil_s / dev_s, png_s / dev_s, dev_b / 1e6, pil_b / 1e6, png_b / 1e6,
                                                                              same, a.images, card))
            assert same == a.images
            del images, pics
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
