"""CPU: the numpy restatement of the PNG filters (tests/png_ref.py) on hand-made rows, the host container, the size bound, and the
length-limited code construction the deflate kernel runs on one lane (sniper_amd/csrc/huff_code.h, compiled here into a stand-alone
program): complete codes within the limit, and whole dynamic blocks that zlib's inflate accepts."""
import io
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import png_ref

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the five filters ------------------------------------------------------------------------------------------------------------
def test_filters_on_a_hand_made_row():
    cur = np.array([10, 20, 30, 13, 18, 40], np.uint8)           # two pixels
    up = np.array([1, 2, 3, 250, 100, 7], np.uint8)
    f = png_ref.filter_row(cur, up)
    assert f[0].tolist() == [10, 20, 30, 13, 18, 40]
    assert f[1].tolist() == [10, 20, 30, 3, 254, 10]             # left of the first pixel is zero; 18 - 20 wraps
    assert f[2].tolist() == [9, 18, 27, (13 - 250) & 255, (18 - 100) & 255, 33]
    assert f[3].tolist() == [10, 19, 29, (13 - ((10 + 250) >> 1)) & 255, (18 - ((20 + 100) >> 1)) & 255, (40 - ((30 + 7) >> 1)) & 255]
    # Paeth of the first pixel: a = c = 0, so the predictor is b
    assert f[4][:3].tolist() == [9, 18, 27]


def test_average_floors_the_nine_bit_sum():
    # the second pixel has left = 255 and up = 255
    f = png_ref.filter_row(np.array([255, 255, 255, 255, 254, 0], np.uint8), np.array([9, 9, 9, 255, 255, 255], np.uint8))
    assert f[3][3:].tolist() == [(255 - 255) & 255, (254 - 255) & 255, (0 - 255) & 255]      # (255 + 255) >> 1 = 255, not 127


def test_the_three_paeth_branches_and_their_tie_order():
    P = lambda a, b, c: int(png_ref.paeth_predictor(np.array([a]), np.array([b]), np.array([c]))[0])
    assert P(100, 20, 20) == 100            # p = 100: pa = 0 -> a
    assert P(20, 100, 20) == 100            # p = 100: pb = 0 -> b
    assert P(10, 30, 20) == 20              # p = 20: pc = 0 -> c
    assert P(200, 100, 150) == 150          # p = 150 -> c
    assert P(2, 6, 0) == 6                  # p = 8: pa = 6, pb = 2, pc = 8 -> b
    assert P(10, 10, 10) == 10              # all three distances equal: a
    assert P(8, 8, 0) == 8                  # p = 16: pa = pb = 8 < pc = 16 -> the tie goes to a
    assert P(0, 0, 4) == 0                  # p = -4: pa = pb = 4 < pc = 8 -> a
    assert P(0, 4, 4) == 0 and P(4, 0, 4) == 0          # p = 0: a nearest; p = 0: b nearest
    assert P(3, 5, 4) == 4                  # p = 4 -> c
    assert P(0, 2, 1) == 1 and P(1, 3, 1) == 3
    # a tie between b and c goes to b: p = a + b - c with pb == pc < pa
    assert P(0, 6, 2) == 6                  # p = 4: pa = 4, pb = 2, pc = 2 -> b


def test_filter_choice_takes_the_lowest_type_among_equal_costs():
    pic = np.zeros((2, 2, 3), np.uint8)                          # every filter costs 0 on both rows: type 0
    stream, types = png_ref.filter_picture(pic, want_types=True)
    assert types == [0, 0] and stream.tolist() == [0] * 14
    pic = np.full((3, 4, 3), 200, np.uint8)                      # first row: Sub beats None; later rows: Up (2) ties Paeth (4)
    stream, types = png_ref.filter_picture(pic, want_types=True)
    assert types == [1, 2, 2]
    assert png_ref.filter_cost([0, 1, 255, 128, 129]) == 0 + 1 + 1 + 128 + 127


# ---- the container ---------------------------------------------------------------------------------------------------------------
def test_container_opens_in_pil_and_equals_the_picture():
    from PIL import Image
    from sniper_amd.png import png_container
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (5, 7), (33, 20)):
        pic = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        data = png_container(h, w, zlib.compress(png_ref.filter_picture(pic).tobytes()))
        assert data[:8] == b'\x89PNG\r\n\x1a\n' and data.count(b'IDAT') == 1
        im = Image.open(io.BytesIO(data))
        assert im.mode == 'RGB' and im.size == (w, h)
        assert np.array_equal(np.asarray(im), pic)


# ---- the size bound --------------------------------------------------------------------------------------------------------------
def test_size_bound_formula():
    from sniper_amd.png import deflate_bound
    B = 32768
    assert deflate_bound(0, B) == 11                             # header 2, one empty stored block 5, Adler-32 4
    assert deflate_bound(1, B) == 1 + 10 + 6
    assert deflate_bound(B, B) == B + 16 and deflate_bound(B + 1, B) == B + 1 + 21
    for n in (0, 1, 2, 3, B - 1, B, B + 1, 2 * B, 2 * B + 1, 10 * B + 5):
        assert deflate_bound(n, B) == png_ref.deflate_bound(n, B)
        nb = -(-n // B)
        # what the coder writes at the most: every block stored (len + 5), or for n = 0 the one empty stored block
        assert 2 + n + 5 * max(nb, 1) + 4 <= deflate_bound(n, B)


def test_size_bound_uses_the_librarys_block_size():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd.png import deflate_bound, deflate_limits
    B = deflate_limits()['block']
    assert 8192 <= B <= 65535
    assert deflate_bound(B + 1) == B + 1 + 5 * 3 + 6


# ---- the code construction, as a stand-alone host program ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def huff(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        from sniper_amd.build import _hipcc
        cxx = _hipcc()
    exe = str(tmp_path_factory.mktemp('huff') / 'png_huff_main')
    subprocess.run([cxx, '-O1', '-std=c++17', '-Wall', os.path.join(HERE, 'png_huff_main.cpp'), '-o', exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input='\n'.join(lines) + '\n', stdout=subprocess.PIPE, text=True, check=True)
        return [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    return run


def _fib_counts(k):
    c = [1, 3]
    while len(c) < k:
        c.append(c[-1] + c[-2])
    return c


def test_limited_codes_are_complete_and_within_the_limit(huff):
    rng = np.random.default_rng(0)
    cases = []
    cases.append((15, _fib_counts(30)))                          # unlimited depth 29
    cases.append((15, [1] * 286))
    cases.append((15, [1, 1]))
    cases.append((15, [5, 0, 0, 7]))
    cases.append((15, [1] + [0] * 200 + [32768]))
    cases.append((15, [2 ** k for k in range(20)]))
    cases.append((7, _fib_counts(19)))                           # the code-length alphabet at its limit
    cases.append((7, [1] * 19))
    cases.append((7, [286, 1]))
    cases.append((7, [100, 0, 0, 3, 9, 27, 81, 1, 1]))
    for _ in range(40):
        n = int(rng.integers(2, 287))
        f = (rng.integers(0, 4, n) * rng.integers(0, 2000, n)).tolist()
        if sum(1 for v in f if v) >= 2:
            cases.append((15, f))
    out = huff(['lens %d %d %s' % (mb, len(f), ' '.join(str(v) for v in f)) for mb, f in cases])
    assert len(out) == len(cases)
    for (mb, f), row in zip(cases, out):
        kraft, lens = row[0], row[1:]
        assert len(lens) == len(f)
        assert all((l > 0) == (v > 0) for l, v in zip(lens, f)), (f, lens)
        assert max(lens) <= mb, (mb, f, lens)
        assert kraft == 1 << mb, (mb, f, lens)                   # complete: neither over-subscribed nor incomplete
        # a rarer symbol never has a shorter code
        used = sorted((v, i) for i, v in enumerate(f) if v)
        assert all(lens[a[1]] >= lens[b[1]] for a, b in zip(used, used[1:])), (f, lens)
    # determinism: the same input twice
    assert huff(['lens 15 30 ' + ' '.join(str(v) for v in _fib_counts(30))] * 2)[0] == out[0]


def _coded(huff, block, final=1):
    toks = png_ref.tokens(block)
    hist = png_ref.histogram(toks)
    row = huff(['block %d %s' % (final, ' '.join(str(v) for v in hist))])[0]
    hb, bits, nw = row[:3]
    words = row[3:3 + nw]
    lens = row[3 + nw:3 + nw + 286]
    codes = row[3 + nw + 286:]
    body = png_ref.pack_dynamic_block(toks, hb, words, lens, codes)
    assert (bits + 7) // 8 == len(body)
    return body, lens, toks


def test_whole_dynamic_blocks_inflate(huff):
    rng = np.random.default_rng(1)
    fib = _fib_counts(16)
    blocks = [
        bytes(rng.integers(0, 4, 5000).astype(np.uint8)),
        bytes(range(256)) * 3,
        b'\x07' * 9000,                                           # one literal, length symbols, 256
        b'ab' * 1000,                                            # no run: no distance code
        b'x' + b'y' * 2 + b'z' * 3 + b'q' * 4 + b'r' * 257 + b's' * 258 + b't' * 259 + b'u' * 260 + b'v' * 261 + b'w' * 262 + b'k' * 517 + b'e',
        bytes(np.clip(rng.normal(128, 3, 20000), 0, 255).astype(np.uint8)),
    ]
    # 16 values with Fibonacci-like counts, no equal neighbours: the unlimited code would be 16 deep
    arr = png_ref.spread(fib)
    assert len(arr) == 5775 and np.bincount(arr).tolist() == fib
    assert all(k == 'l' for k, _ in png_ref.tokens(bytes(arr))) and png_ref.huffman_depth(fib + [1]) == 16
    blocks.append(bytes(arr))
    for blk in blocks:
        body, lens, toks = _coded(huff, blk)
        assert max(lens) <= 15
        assert zlib.decompress(body, -15) == blk


def test_tokens_restate_the_greedy_scan():
    assert png_ref.tokens(b'aaaa') == [('l', 97), ('m', 3)]
    assert png_ref.tokens(b'aaa') == [('l', 97)] * 3                                        # L = 2 at p = 1: literals
    assert png_ref.tokens(b'a' * 260) == [('l', 97), ('m', 258), ('l', 97)]
    assert png_ref.tokens(b'a' * 262) == [('l', 97), ('m', 258), ('m', 3)]
    assert png_ref.tokens(b'ba' * 3) == [('l', 98), ('l', 97)] * 3
    assert [png_ref.length_symbol(L)[0] for L in (3, 10, 11, 12, 13, 257, 258)] == [257, 264, 265, 265, 266, 284, 285]
