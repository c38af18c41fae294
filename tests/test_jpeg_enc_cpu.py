"""CPU: the JPEG encoder's restatement (tests/jpeg_enc_ref.py) against PIL byte for byte, the host functions of sniper_amd/jpeg_encode.py
against PIL's files, and the per-block code of the kernels (sniper_amd/csrc/jpeg_enc_code.h) as a stand-alone host program under the
address and undefined-behaviour sanitizers: the exact reciprocals, the forward DCT and quantisation, the coder at every block's own
bit offset into a buffer of exactly the reported size -- and one byte short, which is refused and not overrun."""
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_enc_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SUBS = ('4:2:0', '4:2:2', '4:4:4')
QUALITIES = (10, 30, 75, 95, 100)


def _scan_of(data):
    """the entropy-coded bytes of a file with one scan"""
    at = data.index(b'\xff\xda')
    n = (data[at + 2] << 8) | data[at + 3]
    assert data[-2:] == b'\xff\xd9'
    return data[at + 2 + n:-2]


# ---- the restatement against PIL ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def grid():
    """[(h, w, kind, grey, quality, subsampling, PIL's file)]: 18 sizes x 3 contents x (3 samplings + grey) x 5 qualities"""
    cases = []
    for h, w in ref.SIZES:
        for kind in ('flat', 'smooth', 'noise'):
            for grey in (False, True):
                pic = ref.picture(kind, h, w, grey)
                for q in QUALITIES:
                    for sub in (SUBS if not grey else ('4:4:4',)):
                        cases.append((h, w, kind, grey, q, sub, pic, ref.pil_encode(pic, q, sub)))
    assert len(cases) == 1080
    return cases


def test_restatement_equals_pil_on_the_grid(grid):
    bad = [(h, w, kind, grey, q, sub) for h, w, kind, grey, q, sub, pic, want in grid if ref.encode(pic, q, sub) != want]
    assert not bad, bad[:10]


def test_restatement_equals_pil_on_the_extremes():
    seen_dc = seen_ac = stuffed = 0
    n = 0
    for kind in ('pixel_checker', 'block_checker'):
        for h, w in ((16, 16), (33, 40), (67, 101)):
            for grey in (False, True):
                pic = ref.picture(kind, h, w, grey)
                for q in (1, 75, 100):
                    for sub in (SUBS if not grey else ('4:4:4',)):
                        want = ref.pil_encode(pic, q, sub)
                        assert ref.encode(pic, q, sub) == want, (kind, h, w, grey, q, sub)
                        n += 1
                        b = ref.blocks(pic, q, sub)
                        comps = ref.block_components(len(b), grey, sub)
                        for c in range(3):
                            dc = b[comps == c, 0]
                            if dc.size:
                                seen_dc = max(seen_dc, int(np.abs(np.diff(np.concatenate([[0], dc]))).max()).bit_length())
                        seen_ac = max(seen_ac, int(np.abs(b[:, 1:]).max()).bit_length())
                        stuffed = max(stuffed, _scan_of(want).count(b'\xff\x00'))
    assert n == 72
    assert seen_dc == 11 and seen_ac == 10 and stuffed >= 24, (seen_dc, seen_ac, stuffed)


def test_default_save_is_quality_75_420():
    from PIL import Image
    pic = ref.picture('smooth', 33, 40)
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, 'JPEG')
    assert buf.getvalue() == ref.encode(pic) == ref.pil_encode(pic, 75, '4:2:0')


def test_the_grid_is_not_vacuous(grid):
    stuffed = f0 = fill = 0
    dummies = set()
    for h, w, kind, grey, q, sub, pic, want in grid:
        s = _scan_of(want)
        stuffed += s.count(b'\xff\x00')
        if kind == 'flat' and q != 75:
            continue          # (the rest is slow in Python and adds nothing)
        b, dummy = ref.blocks(pic, q, sub, want_dummy=True)
        comps = ref.block_components(len(b), grey, sub)
        _, sizes = ref.scan(b, comps, want_bits=True)
        fill += sum(sizes) % 8 != 0
        for blk, c in zip(b, comps):
            nz = np.flatnonzero(blk[1:])
            gaps = np.diff(np.concatenate([[-1], nz]))
            f0 += int((gaps > 16).any())
        if not grey and sub == '4:2:0':
            for m in range(0, len(dummy), 6):          # the dummy luma blocks of each MCU, as (x, y) inside it
                dummies.add(frozenset((bx, by) for is_dummy, bx, by in dummy[m:m + 4] if is_dummy))
    assert stuffed > 0 and f0 > 0 and fill > 0
    # an MCU with dummies to the right only, below only, and in both directions (the corner)
    assert dummies >= {frozenset(), frozenset({(1, 0), (1, 1)}), frozenset({(0, 1), (1, 1)}), frozenset({(1, 0), (0, 1), (1, 1)})}, dummies


def test_edge_rule_differs_from_padding_the_input():
    # 24 x 50 and 8 x 8 in 4:2:0: the chroma plane is NOT what downsampling an edge-padded picture gives
    differs = 0
    for h, w in ((24, 50), (8, 8)):
        pic = ref.picture('noise', h, w)
        mw, mh = -(-w // 16), -(-h // 16)
        padded = np.pad(pic, ((0, 16 * mh - h), (0, 16 * mw - w), (0, 0)), mode='edge')
        a = ref.component_samples(pic, '4:2:0')[1]
        b = ref.component_samples(padded, '4:2:0')[1]
        assert a.shape == b.shape
        differs += int(not np.array_equal(a, b))
        assert ref.encode(pic) == ref.pil_encode(pic)
    assert differs >= 1


def test_fdct_in_32_bits_equals_64_bits_on_the_extremes():
    rng = np.random.default_rng(5)
    blocks = [np.full((8, 8), v) for v in (-128, 127)]
    yy, xx = np.mgrid[0:8, 0:8]
    for ky in range(8):                    # the sign patterns of every basis function: the largest value of each coefficient
        for kx in range(8):
            s = np.cos((2 * yy + 1) * ky * np.pi / 16) * np.cos((2 * xx + 1) * kx * np.pi / 16)
            blocks += [np.where(s >= 0, 127, -128), np.where(s >= 0, -128, 127)]
    blocks += [rng.choice([-128, 127], (8, 8)) for _ in range(2000)]
    blocks = np.array(blocks, np.int64)
    wide = ref.fdct(blocks, np.int64)
    narrow = ref.fdct(blocks, np.int32)          # (a wrap in 32 bits would give another value)
    assert narrow.dtype == np.int32 and np.array_equal(wide, narrow)
    assert np.abs(wide).max() == 8192 and wide[0, 0, 0] == -8192 and wide[1, 0, 0] == 8128
    # AC category 10 at the most after the finest quantisation (divisor 8)
    assert (np.abs(wide.reshape(len(wide), 64)[:, 1:]).max() + 4) // 8 < 1024


# ---- the host functions of the package ------------------------------------------------------------------------------------------------------
def test_quant_tables_and_header_against_pil():
    from PIL import Image
    from sniper_amd.jpeg_encode import ZIGZAG, jpeg_header, jpeg_quant_tables
    pic, grey = ref.picture('smooth', 17, 33), ref.picture('smooth', 17, 33, grey=True)
    for q in (1, 10, 30, 49, 50, 75, 95, 100):
        t = jpeg_quant_tables(q)
        assert t.shape == (2, 64) and t.min() >= 1 and t.max() <= 255
        data = ref.pil_encode(pic, q, '4:2:0')
        qt = Image.open(io.BytesIO(data)).quantization
        for i in (0, 1):
            mine = [int(t[i][z]) for z in ZIGZAG]
            theirs = list(qt[i])
            # (Pillow hands the tables out in the file's order or in natural order, depending on its version)
            assert theirs == mine or theirs == [int(v) for v in t[i]], (q, i)
        for sub in SUBS:
            data = ref.pil_encode(pic, q, sub)
            head = jpeg_header(17, 33, q, sub)
            assert data[:len(head)] == head and head == ref.header(17, 33, q, sub), (q, sub)
            assert data[len(head):-2] == _scan_of(data)
        # (grey: the sampling is ignored and the header says 1 x 1, which is PIL's file when it is told nothing or 4:4:4; told
        # 4:2:0, libjpeg writes that factor into the header of the same scan)
        data = ref.pil_encode(grey, q, '4:4:4')
        head = jpeg_header(17, 33, q, grey=True)
        assert data[:len(head)] == head and head.count(b'\xff\xc4') == 2 and head.count(b'\xff\xdb') == 1


def test_requests_outside_the_parameters_are_refused():
    from sniper_amd import jpeg_encode as je
    pic = ref.picture('flat', 8, 8)
    for kw in (dict(quality=0), dict(quality=101), dict(quality='keep'), dict(quality='web_high'), dict(quality=75.5),
               dict(subsampling='4:1:1'), dict(subsampling=2)):
        with pytest.raises(ValueError):
            je.encode_jpeg([pic], **kw)
    for bad in (np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32), np.zeros((0, 8, 3), np.uint8), np.zeros((8,), np.uint8)):
        with pytest.raises(ValueError):
            je.encode_jpeg([pic, bad])
    with pytest.raises(ValueError):
        je.encode_jpeg([])
    with pytest.raises(ValueError):
        je.jpeg_header(70000, 8)
    with pytest.raises(ValueError):
        je.write_jpeg(['a.jpg', 'b.jpg'], [pic])


# ---- the per-block code as a stand-alone program under the sanitizers -------------------------------------------------------------------
@pytest.fixture(scope='module')
def program(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        from sniper_amd.build import _hipcc
        cxx = _hipcc()
    exe = str(tmp_path_factory.mktemp('jpeg_enc') / 'jpeg_enc_main')
    cmd = [cxx, '-O1', '-g', '-std=c++17', '-Wall', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
           os.path.join(HERE, 'jpeg_enc_main.cpp'), '-o', exe]
    # the sanitizers' runtimes linked into the program itself (clang's default; gcc takes two flags for it)
    if subprocess.run(cmd + ['-static-libasan', '-static-libubsan'], stderr=subprocess.DEVNULL).returncode != 0:
        subprocess.run(cmd, check=True)

    def run(text):
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, r.stderr[-4000:]          # (a sanitizer report fails the run)
        return r.stdout.splitlines()
    return run


def test_reciprocal_division_is_exact(program):
    pairs, bad = (int(v) for v in program('recip\n')[0].split())
    assert pairs == 255 * 16385 + 2033 * 16384 and bad == 0
    # the same statement in numpy
    d = np.arange(8, 2041, dtype=np.uint64)[:, None]
    n = np.arange(0, 8192 + 1020 + 1, dtype=np.uint64)[None, :]
    m = (np.uint64(1) << np.uint64(32)) // d + np.uint64(1)
    assert np.array_equal((n * m) >> np.uint64(32), n // d)


def _program_cases():
    cases = []
    for h, w in ((8, 8), (17, 16), (16, 17), (24, 50), (31, 3)):
        for kind, q in (('smooth', 75), ('noise', 100), ('pixel_checker', 100), ('block_checker', 1)):
            for grey, sub in ((False, '4:2:0'), (False, '4:2:2'), (False, '4:4:4'), (True, '4:4:4')):
                cases.append((ref.picture(kind, h, w, grey), q, sub, grey))
    return cases


def test_program_transform_and_quantisation_equal_the_restatement(program):
    jobs, want = [], []
    for pic, q, sub, grey in _program_cases():
        for ci, plane in enumerate(ref.component_samples(pic, sub)):
            hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
            blk = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
            jobs.append('quant %d %d %d\n%s\n' % (q, 1 if ci else 0, len(blk), ' '.join(str(v) for v in blk.reshape(-1))))
            table = ref.quant_table(ref.QUANT_CHROMA if ci else ref.QUANT_LUMA, q)
            want.append(ref.quantise(ref.fdct(blk.reshape(-1, 8, 8) - 128), table).reshape(-1, 64)[:, ref.ZIGZAG].reshape(-1))
    out = program(''.join(jobs))
    assert len(out) == len(want) > 100
    for line, w in zip(out, want):
        assert np.array_equal(np.array(line.split(), np.int64), w)


def _scan_jobs(short):
    jobs, want = [], []
    for pic, q, sub, grey in _program_cases():
        b = ref.blocks(pic, q, sub)
        comps = ref.block_components(len(b), grey, sub)
        hs, vs = (1, 1) if grey else ref.SAMPLINGS[sub]
        jobs.append('scan %d %d %d %d\n%s\n' % (len(b), hs * vs, hs * vs + (0 if grey else 2), short, ' '.join(str(v) for v in b.reshape(-1))))
        want.append(ref.scan(b, comps, want_bits=True))
    return jobs, want


def test_program_codes_every_block_at_its_own_offset_into_exactly_the_reported_size(program):
    jobs, want = _scan_jobs(0)
    out = program(''.join(jobs))
    assert len(out) == 3 * len(jobs)
    for i, (scan, sizes) in enumerate(want):
        err, nbytes = (int(v) for v in out[3 * i].split())
        assert err == 0 and [int(v) for v in out[3 * i + 1].split()] == sizes
        assert nbytes == (sum(sizes) + 7) // 8
        raw = bytes.fromhex(out[3 * i + 2])
        assert len(raw) == nbytes and raw.replace(b'\xff', b'\xff\x00') == scan, i
        assert max(sizes) <= 22 + 63 * 26


def test_program_refuses_a_capacity_one_byte_short_and_does_not_overrun(program):
    jobs, want = _scan_jobs(1)
    out = program(''.join(jobs))          # (the buffer has exactly the capacity: the sanitizer would report the byte behind it)
    for i, (scan, sizes) in enumerate(want):
        err, nbytes = (int(v) for v in out[3 * i].split())
        assert err & 1, i                  # SNE_NO_ROOM
        kept = bytes.fromhex(out[3 * i + 2])
        raw = scan.replace(b'\xff\x00', b'\xff')
        assert len(kept) == (nbytes + 3) // 4 * 4 - 4 and kept == raw[:len(kept)]          # what had room is what belongs there
