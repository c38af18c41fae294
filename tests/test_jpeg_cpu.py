"""CPU: the JPEG decoder's restatement (tests/jpeg_ref.py) against PIL bit for bit, the parser's classification, the entropy decoder
of the kernel (sniper_amd/csrc/jpeg_entropy.h) as a stand-alone host program under the address and undefined-behaviour sanitizers --
sound, truncated and overwritten streams, sequentially and by the kernel's rounds -- and the default wiring, which calls none of it."""
import contextlib
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ref
from jpeg_util import SAMPLINGS, VARIANTS, encode, picture, pil_bgr, small_damaged_streams

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((1, 1), (8, 8), (9, 17), (16, 16), (17, 33), (67, 101), (31, 2), (2, 31), (48, 64))


# ---- the restatement against PIL -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w', SIZES)
def test_restatement_equals_pil_bit_for_bit(h, w):
    from sniper_amd.jpeg import parse_jpeg
    decoded = 0
    for kind in ('smooth', 'noise'):
        arr = picture(kind, h, w)
        for sname, samp in SAMPLINGS:
            for q in (30, 75, 95, 100):
                for vname, kw in VARIANTS:
                    data = encode(arr, samp, q, **kw)
                    head = parse_jpeg(data)
                    if samp in (1, 2) and w <= 2:
                        # a subsampled chroma plane one sample wide: libjpeg's edge code reads the padding column -- not decoded here
                        assert head == {'fallback': 'narrow_chroma'}, (h, w, sname, head)
                        continue
                    assert 'fallback' not in head, (h, w, kind, sname, q, vname, head)
                    got = jpeg_ref.decode_bgr(data, head)
                    assert np.array_equal(got, pil_bgr(data)), (h, w, kind, sname, q, vname)
                    decoded += 1
    assert decoded == (128 if w > 2 else 64)


def test_chroma_two_samples_wide_is_replicated():
    # libjpeg keeps its triangle filters for planes wider than two samples
    for h, w in ((31, 3), (3, 31), (5, 4)):
        for samp in (1, 2):
            data = encode(picture('noise', h, w), samp, 95)
            assert np.array_equal(jpeg_ref.decode_bgr(data), pil_bgr(data)), (h, w, samp)


# ---- the parser ------------------------------------------------------------------------------------------------------------------
def test_parser_classifies_what_the_device_does_not_decode():
    from PIL import Image
    from sniper_amd.jpeg import parse_jpeg
    arr = picture('smooth', 24, 40)
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, 'JPEG', progressive=True)
    assert parse_jpeg(buf.getvalue()) == {'fallback': 'progressive'}
    buf = io.BytesIO()
    Image.fromarray(np.dstack([arr, arr[:, :, :1]]), 'CMYK').save(buf, 'JPEG')
    assert parse_jpeg(buf.getvalue())['fallback'] in ('cmyk', 'adobe')
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, 'PNG')
    assert parse_jpeg(buf.getvalue()) == {'fallback': 'not_jpeg'}
    assert parse_jpeg(b'') == {'fallback': 'not_jpeg'}
    assert parse_jpeg(encode(arr, 2)[:100])['fallback'] == 'damaged_header'
    # a sampling the kernels do not take: the 4:2:0 header rewritten to 1 x 2 luma
    data = bytearray(encode(arr, 2))
    at = data.index(b'\xff\xc0')
    assert data[at + 11] == 0x22
    data[at + 11] = 0x12
    assert parse_jpeg(bytes(data)) == {'fallback': 'sampling'}


def test_parser_reads_headers_tables_and_segments():
    from sniper_amd.jpeg import parse_jpeg
    arr = picture('noise', 40, 56)
    g = parse_jpeg(encode(arr, None, 75))
    assert (g['H'], g['W'], g['ncomp'], g['hs'], g['vs'], g['bpm'], g['mcux'], g['mcuy'], g['ri']) == (40, 56, 1, 1, 1, 1, 7, 5, 0)
    c = parse_jpeg(encode(arr, 2, 75))
    assert (c['ncomp'], c['hs'], c['vs'], c['bpm'], c['mcux'], c['mcuy'], c['n_mcu']) == (3, 2, 2, 6, 4, 3, 12)
    assert c['sel'] == 0b111100 and len(c['seg_first']) == 1 and c['qtab'].shape == (3, 64)
    assert c['qtab'][0, 0] == 8 and c['qtab'][1, 0] == 9          # the standard tables at quality 75, the DC entries
    # the standard and the optimised code: other tables, the same coefficients
    o = parse_jpeg(encode(arr, 2, 75, optimize=True))
    assert not np.array_equal(o['dht'], c['dht'])
    assert np.array_equal(jpeg_ref.coefficients(o, encode(arr, 2, 75, optimize=True)), jpeg_ref.coefficients(c, encode(arr, 2, 75)))
    # DRI: one MCU per interval, the markers excluded from the segments
    data = encode(arr, 2, 75, restart_marker_blocks=1)
    r = parse_jpeg(data)
    assert r['ri'] == 1 and len(r['seg_first']) == 12
    for s in range(11):
        e = int(r['seg_end'][s])
        assert data[e] == 0xff and data[e + 1] == 0xd0 + (s & 7) and int(r['seg_first'][s + 1]) == e + 2
    assert data[int(r['seg_end'][-1]):int(r['seg_end'][-1]) + 2] == b'\xff\xd9'
    rows = parse_jpeg(encode(arr, 2, 75, restart_marker_rows=1))
    assert rows['ri'] == 4 and len(rows['seg_first']) == 3
    # a restart marker out of order is the host's to find
    bad = bytearray(data)
    bad[int(r['seg_end'][2]) + 1] = 0xd5
    assert parse_jpeg(bytes(bad)) == {'fallback': 'damaged_markers'}


# ---- the entropy decoder as a stand-alone program under the sanitizers -----------------------------------------------------------------
@pytest.fixture(scope='module')
def entropy(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        from sniper_amd.build import _hipcc
        cxx = _hipcc()
    exe = str(tmp_path_factory.mktemp('jpeg') / 'jpeg_entropy_main')
    cmd = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           os.path.join(HERE, 'jpeg_entropy_main.cpp'), '-o', exe]
    # the sanitizers' runtimes linked into the program itself (clang's default; gcc takes two flags for it)
    if subprocess.run(cmd + ['-static-libasan', '-static-libubsan'], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)

    def run(jobs):
        """jobs: lists of four lines -> per job (status, blocks, rounds per segment, coefficients or None)"""
        r = subprocess.run([exe], input='\n'.join('\n'.join(j) for j in jobs) + '\n', stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        lines, out = r.stdout.splitlines(), []
        for j in jobs:
            head = [int(v) for v in lines.pop(0).split()]
            coef = np.array(lines.pop(0).split(), np.int64) if j[0].split()[-1] == '1' else None
            out.append((head[0], head[1], head[2:], coef))
        assert not lines
        return out
    return run


def _nsub(head, sub):
    return [max(1, -(-(int(b) - int(a)) // sub)) for a, b in zip(head['seg_first'], head['seg_end'])]


def test_entropy_program_equals_the_restatement_sequentially_and_by_rounds(entropy):
    from sniper_amd.jpeg import parse_jpeg
    cases = []
    for h, w in ((8, 8), (17, 33), (48, 64)):
        for kind in ('smooth', 'noise'):
            for sname, samp in SAMPLINGS:
                for q in (30, 100):
                    for vname, kw in VARIANTS:
                        data = encode(picture(kind, h, w), samp, q, **kw)
                        cases.append((data, parse_jpeg(data)))
    modes = (('seq', 64), ('rounds', 16), ('rounds', 64))
    out = entropy([jpeg_ref.entropy_job(head, data, mode, sub) for data, head in cases for mode, sub in modes])
    for i, (data, head) in enumerate(cases):
        want = jpeg_ref.coefficients(head, data).reshape(-1)
        for j, (mode, sub) in enumerate(modes):
            status, blocks, rounds, coef = out[3 * i + j]
            assert status == 0 and blocks == head['n_mcu'] * head['bpm'], (i, mode, sub, status)
            assert np.array_equal(coef, want), (i, mode, sub)
            if mode == 'rounds':
                assert all(1 <= r <= n for r, n in zip(rounds, _nsub(head, sub))), (rounds, _nsub(head, sub))


def test_damaged_streams_yield_a_status_and_no_bad_access(entropy):
    from sniper_amd.jpeg import parse_jpeg
    data = encode(picture('noise', 16, 24, seed=3), 2, 85)
    head = parse_jpeg(data)
    first, end = int(head['scan']), int(head['seg_end'][-1])
    jobs, kinds = [], []
    for n in range(first, end + 1):                        # truncated at every byte from the scan's first on
        cut = data[:n]
        h = parse_jpeg(cut)
        assert 'fallback' not in h and int(h['seg_end'][-1]) == n
        for mode in ('seq', 'rounds'):
            jobs.append(jpeg_ref.entropy_job(h, cut, mode, 16, want_coef=False))
            kinds.append(('cut', n, mode))
    rng = np.random.default_rng(4)
    for n in range(first, end):                            # every byte of the scan overwritten, three ways
        for v in (data[n] ^ 0xff, data[n] ^ 0x10, int(rng.integers(0, 256))):
            bad = bytearray(data)
            bad[n] = v
            h = parse_jpeg(bytes(bad))
            if 'fallback' in h:                            # the byte made a marker: the host's parser has it
                continue
            for mode in ('seq', 'rounds'):
                jobs.append(jpeg_ref.entropy_job(h, bytes(bad), mode, 16, want_coef=True))
                kinds.append(('over', n, mode))
    for name, bad in small_damaged_streams():              # what the GPU tests decode
        h = parse_jpeg(bad)
        assert 'fallback' not in h, name
        for mode, sub in (('seq', 128), ('rounds', 128), ('rounds', 16)):
            jobs.append(jpeg_ref.entropy_job(h, bad, mode, sub, want_coef=False))
            kinds.append((name, 0, mode))
    out = entropy(jobs)                                    # (a sanitizer report fails the run)
    assert len(out) == len(jobs) > 500
    for (kind, n, mode), (status, blocks, rounds, coef) in zip(kinds, out):
        if kind == 'cut' and n <= end - 2:
            assert status != 0, (kind, n, mode)
        if kind in ('truncated', 'overwritten', 'more_blocks'):
            assert status != 0, (kind, mode)
    # the rounds find what the sequential decode finds; a stream both take as sound decodes alike
    for i in range(0, len(out) - 9, 2):
        a, b = out[i], out[i + 1]
        assert (a[0] == 0) == (b[0] == 0), kinds[i]
        if a[0] == 0 and a[3] is not None:
            assert np.array_equal(a[3], b[3]), kinds[i]


def test_rounds_end_within_the_subsequence_count_when_no_guess_ever_synchronises(entropy):
    # one code of one bit in either table: DC category 0 = '0', AC (run 0, size 1) = '0' and its bit '0' = -1.  Every block is 127
    # zero bits, the stream is all zeros, and a decode started anywhere is valid -- in its own phase for ever: no chain started from
    # a guess meets the true one, and only the true entry, passed on one subsequence per round, ends the rounds.
    dht = np.zeros((4, 272), np.uint8)
    dht[0, 0], dht[0, 16] = 1, 0
    dht[2, 0], dht[2, 16] = 1, 0x01
    blocks, sub = 48, 16
    nbytes = blocks * 127 // 8
    assert blocks * 127 == nbytes * 8
    head = dict(bpm=3, hs=1, vs=1, sel=0, ri=0, n_mcu=blocks // 3, dht=dht, seg_first=[0], seg_end=[nbytes])
    nsub = -(-nbytes // sub)
    seq, par = entropy([jpeg_ref.entropy_job(head, bytes(nbytes), 'seq', sub), jpeg_ref.entropy_job(head, bytes(nbytes), 'rounds', sub)])
    want = np.full((blocks, 64), -1, np.int64)
    want[:, 0] = 0
    assert seq[0] == 0 and seq[1] == blocks and np.array_equal(seq[3], want.reshape(-1))
    assert par[0] == 0 and par[1] == blocks and np.array_equal(par[3], seq[3])
    assert par[2] == [nsub]                                # as many rounds as subsequences, and not one more


# ---- the C ABI refuses what its tables do not bear out ---------------------------------------------------------------------------------
def test_entry_points_refuse_inconsistent_tables_before_any_launch():
    import ctypes
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import SniperHipError, lib
    from sniper_amd.jpeg import jpeg_limits
    lim = jpeg_limits()
    assert lim['img_fields'] == 16 and lim['seg_fields'] == 8 and lim['min_sub'] == 16 <= lim['sub'] <= 4096 and lim['max_bpm'] == 6
    P = ctypes.c_void_p(64)
    # one 16 x 16 4:2:0 image: 1 MCU of 6 blocks, one segment of 100 bytes
    img = np.array([[16, 16, 3, 2, 2, 1, 1, 6, 0, 1, 0, 0, 0, 120, 0b111100, 0]], np.int32)
    seg = np.array([[0, 20, 120, 0, 1, 0, 0, 0]], np.int32)

    def entropy_call(img=img, seg=seg, sub=128, n_sub=1, n_blocks=6, total=120, phases=3, I=1, S=1):
        hp = lambda a: ctypes.c_void_p(a.ctypes.data)
        return ('sn_jpeg_entropy', P, total, P, hp(img), I, P, hp(seg), S, P, sub, n_sub, n_blocks, P, P, P, P, P, phases, None)

    def refused(call, *words):
        with pytest.raises(SniperHipError) as e:
            lib().call(*call)
        assert (call[0] + ':') in str(e.value) and all(w in str(e.value) for w in words), str(e.value)

    refused(entropy_call(sub=8), 'sub_bytes')
    refused(entropy_call(phases=0), 'phases')
    refused(entropy_call(total=100), 'stream', 'total_bytes')
    refused(entropy_call(n_blocks=7), 'n_blocks')
    refused(entropy_call(n_sub=2), 'n_sub')
    refused(entropy_call(sub=64), 'subsequences')                       # 100 bytes are two subsequences of 64
    bad = img.copy()
    bad[0, 7] = 4
    refused(entropy_call(img=bad), 'MCU grid')
    bad = img.copy()
    bad[0, 3:5] = (1, 2)
    refused(entropy_call(img=bad), 'sampling')
    bad = seg.copy()
    bad[0, 2] = 121
    refused(entropy_call(seg=bad), 'segment 0')
    long_img, long_seg = img.copy(), seg.copy()                          # a scan of 16385 subsequences of 16 bytes
    long_img[0, 13] = long_seg[0, 2] = 20 + 16385 * 16
    long_seg[0, 4] = 16385
    refused(entropy_call(img=long_img, seg=long_seg, sub=16, n_sub=16385, total=20 + 16385 * 16), 'segment 0', '16384')
    bad = img.copy()
    bad[0, 0] = 2
    bad[0, 5] = 1
    refused(entropy_call(img=bad), 'one sample wide')
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    refused(('sn_jpeg_pixels', P, hp(img), 1, P, P, 6, P, 100, P, P, None), 'planes', 'plane_bytes')
    refused(('sn_jpeg_pixels', P, hp(img), 1, None, P, 6, P, 384, P, P, None), 'null')
    refused(('sn_jpeg_dc', P, hp(img), 1, P, hp(seg), 2, 6, P, P, None), 'segments')


# ---- the default wiring calls none of it ---------------------------------------------------------------------------------------------
def test_default_caches_and_decode_ahead_make_no_jpeg_call(tmp_path, monkeypatch):
    import torch
    from sniper_amd import hip, jpeg
    from sniper_amd.data import im_worker as iw
    calls = []
    real = hip.call
    monkeypatch.setattr(hip, 'call', lambda name, *a: calls.append(name) or real(name, *a))
    monkeypatch.setattr(jpeg, 'decode_jpeg', lambda *a, **k: calls.append('decode_jpeg'))
    monkeypatch.setattr(iw, '_to_device', lambda im: torch.as_tensor(im))          # (no GPU here: the upload is not what is tested)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(torch.cuda, 'current_stream', lambda *a: None)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda *a: None)
    monkeypatch.setattr(torch.cuda, 'stream', lambda s: contextlib.nullcontext())
    monkeypatch.delenv('SNIPER_IMAGE_DECODER', raising=False)
    paths = []
    for i in range(3):
        paths.append(str(tmp_path / ('im%d.jpg' % i)))
        with open(paths[-1], 'wb') as fh:
            fh.write(encode(picture('smooth', 16 + i, 24), 2))
    cache = iw.DeviceImageCache()
    assert cache.decoder == 'pil' and iw.image_decoder() == 'pil'

    class Cfg(object):          # a config from before the key existed
        class network(object):
            PIXEL_MEANS = (0, 0, 0)

        class TRAIN(object):
            SCALES = [(16, 24)]
    worker = iw.im_worker(Cfg, crop_size=16)
    assert worker._cache.decoder == 'pil'
    iw.decode_ahead(worker, paths, threads=2)
    assert all(worker._cache.holds(p) for p in paths)
    got = cache.get_many(paths)
    assert [tuple(g.shape) for g in got] == [(16, 24, 3), (17, 24, 3), (18, 24, 3)]
    assert np.array_equal(got[1].numpy(), pil_bgr(open(paths[1], 'rb').read()))
    assert not [c for c in calls if c.startswith('sn_jpeg') or c == 'decode_jpeg'], calls
    # the three ways to choose, and their order
    Cfg.IMAGE_DECODER = 'device'
    assert iw.DeviceImageCache(cfg=Cfg).decoder == 'device' and iw.DeviceImageCache(cfg=Cfg, decoder='pil').decoder == 'pil'
    del Cfg.IMAGE_DECODER
    monkeypatch.setenv('SNIPER_IMAGE_DECODER', 'device')
    assert iw.DeviceImageCache().decoder == 'device' and iw.DeviceImageCache(decoder='pil').decoder == 'pil'
    with pytest.raises(ValueError):
        iw.DeviceImageCache(decoder='cv2')
