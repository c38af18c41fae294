"""CPU: the restatement of the PNG decoder (tests/png_dec_ref.py) against PIL over the whole matrix of colour types, depths and
filters; parse_png's fields and every fallback reason; the zlib decoder the inflate kernel runs (sniper_amd/csrc/inflate_code.h),
compiled into a stand-alone program -- a second time under the address and undefined-behaviour sanitizers -- against
zlib.decompress on a stream set whose coverage is asserted; and the numpy restatement of the reference's parse_inst."""
import struct
import zlib

import numpy as np
import pytest

import png_dec_ref as ref


# ---- the restatement against PIL -------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files():
    return ref.matrix_files() + ref.special_files()


def test_restatement_equals_pil_on_the_whole_matrix(files):
    seen = set()
    for name, d in files:
        f = ref.read_png(d)
        assert np.array_equal(ref.decode_ref(d), ref.pil_bgr(d)), name
        if f['ctype'] in (0, 3):
            assert np.array_equal(ref.decode_ref(d, 'index'), ref.pil_index(d)), name
        types = np.frombuffer(zlib.decompress(f['idat']), np.uint8)[::ref.row_bytes(f['w'], f['depth'], f['ctype']) + 1]
        seen.add((f['ctype'], f['depth'], (f['h'], f['w']), int(types[0])))
    # every colour type x depth x size, with every filter on its FIRST row
    for ctype, depth in ref.COMBOS:
        for size in ref.SIZES:
            assert {ft for c, d, s, ft in seen if (c, d, s) == (ctype, depth, size)} == {0, 1, 2, 3, 4}, (ctype, depth, size)
    names = {n for n, _ in files}
    assert {'pil_default', 'pil_optimize', 'pil_level0', 'pil_level1', 'idat_1byte', 'rgb_trns_gama', 'short_plte_d4', 'grey_trns'} <= names
    one = dict(files)['idat_1byte']
    assert ref.read_png(one)['kinds'].count(b'IDAT') == len(ref.read_png(one)['idat']) > 50
    # rows with padding bits: 13 pixels of depth 1 and 2 fill 2 and 4 bytes with 3 and 6 bits to spare
    assert ref.row_bytes(13, 1, 0) == 2 and ref.row_bytes(13, 2, 3) == 4 and ref.row_bytes(1, 1, 0) == 1


def test_unfilter_on_hand_made_rows():
    # two pixels of bpp 3; Average floors the 9-bit sum; Paeth's ties go a, b, c
    raw = bytes([1, 10, 20, 30, 3, 254, 10]) + bytes([3, 255, 255, 255, 0, 0, 0]) + bytes([4, 1, 1, 1, 1, 1, 1])
    rows = ref.unfilter(raw, 3, 6, 3)
    assert rows[0].tolist() == [10, 20, 30, 13, 18, 40]
    assert rows[1].tolist() == [(255 + 5) & 255, (255 + 10) & 255, (255 + 15) & 255, (4 + 13) >> 1, (9 + 18) >> 1, (14 + 40) >> 1]
    assert ref.paeth(8, 8, 0) == 8 and ref.paeth(0, 6, 2) == 6 and ref.paeth(10, 30, 20) == 20 and ref.paeth(10, 10, 10) == 10
    assert ref.filter_rows(rows, [1, 3, 4], 3) == raw
    assert ref.unfilter(bytes([0, 255, 3, 255]), 2, 1, 1).tolist() == [[255], [(255 + ((0 + 255) >> 1)) & 255]]
    assert ref.unfilter(bytes([0, 255, 255, 3, 0, 1]), 2, 2, 1)[1].tolist() == [127, (1 + ((127 + 255) >> 1)) & 255]          # 382 >> 1 = 191
    with pytest.raises(ValueError):
        ref.unfilter(bytes([5, 0]), 1, 1, 1)


# ---- parse_png -------------------------------------------------------------------------------------------------------------------
def test_parse_png_fields():
    from sniper_amd.png_decode import parse_png
    rng = np.random.default_rng(1)
    pal = ref.palette_for(rng, 4, short=True)
    rows = ref.random_rows(rng, 9, 13, 4, 3)
    data = ref.png_bytes(13, 9, 4, 3, rows, [4] * 9, palette=pal, idat_split=5, before_idat=[(b'tRNS', b'\x01')])
    h = parse_png(data)
    assert (h['W'], h['H'], h['depth'], h['ctype'], h['channels'], h['row'], h['bpp'], h['raw_len']) == (13, 9, 4, 3, 1, 7, 1, 9 * 8)
    assert h['palette'].shape == (256, 3) and h['plen'] == len(pal) == 7
    assert np.array_equal(h['palette'][:7], pal) and not h['palette'][7:].any()
    assert h['idat'] == ref.read_png(data)['idat'] and zlib.decompress(h['idat']) == ref.filter_rows(rows, [4] * 9, 1)
    h = parse_png(ref.png_bytes(5, 3, 16, 6, ref.random_rows(rng, 3, 5, 16, 6)))
    assert (h['channels'], h['row'], h['bpp'], h['raw_len'], h['plen']) == (4, 40, 8, 3 * 41, 0)
    h = parse_png(ref.png_bytes(13, 2, 1, 0, ref.random_rows(rng, 2, 13, 1, 0)), mode='index')
    assert (h['row'], h['bpp']) == (2, 1)


def test_parse_png_names_every_fallback_reason():
    from sniper_amd.png_decode import parse_png
    rng = np.random.default_rng(2)
    pix = rng.integers(0, 256, (6, 7, 3)).astype(np.uint8)
    rows = pix.reshape(6, -1)
    good = ref.png_bytes(7, 6, 8, 2, rows)
    assert 'fallback' not in parse_png(good)
    reason = lambda d, **k: parse_png(d, **k).get('fallback')
    assert reason(ref.adam7_png_bytes(pix, 2)) == 'interlaced'
    assert reason(ref.png_bytes(7, 6, 16, 0, ref.random_rows(rng, 6, 7, 16, 0))) == 'gray16'
    assert reason(ref.png_bytes(7, 6, 16, 4, ref.random_rows(rng, 6, 7, 16, 4))) == 'gray16'
    assert reason(ref.png_bytes(7, 6, 8, 2, rows, before_idat=[(b'acTL', struct.pack('>II', 1, 0))])) == 'apng'
    no_idat = ref.SIGNATURE + ref.chunk(b'IHDR', struct.pack('>IIBBBBB', 7, 6, 8, 2, 0, 0, 0)) + ref.chunk(b'IEND', b'')
    assert reason(no_idat) == 'no_idat'
    assert reason(good[:-5]) == 'truncated' and reason(good[:40]) == 'truncated' and reason(good[:-12]) == 'truncated'
    assert reason(b'\x89PNG') == 'truncated' and reason(b'') == 'truncated'
    assert reason(b'\xff\xd8\xff\xe0' + good[4:]) == 'bad_header'
    assert reason(ref.png_bytes(7, 6, 3, 2, zdata=zlib.compress(b''))) == 'bad_header'                     # no such depth
    assert reason(ref.png_bytes(7, 6, 8, 5, zdata=zlib.compress(b''))) == 'bad_header'                     # no such colour type
    assert reason(ref.png_bytes(0, 6, 8, 2, zdata=zlib.compress(b''))) == 'bad_header'
    assert reason(ref.png_bytes(7, 6, 8, 3, rows[:, :7])) == 'bad_header'              # a palette image without PLTE
    assert reason(ref.png_bytes(7, 6, 8, 2, rows, interlace=2)) == 'bad_header'
    assert reason(ref.SIGNATURE + ref.chunk(b'IDAT', b'') + good[8:]) == 'bad_header'  # IHDR is not first
    assert reason(ref.png_bytes(7, 6, 8, 2, rows, after_idat=[(b'IDAT', b'')])[:-12] + ref.chunk(b'tEXt', b'a\0b') + ref.chunk(b'IDAT', b'') +
                  ref.chunk(b'IEND', b'')) == 'bad_header'                             # IDAT chunks that are not consecutive
    assert reason(ref.png_bytes(7, 6, 8, 3, rows[:, :7], palette=ref.palette_for(rng, 8), after_idat=[(b'PLTE', b'\0\0\0')])) == 'bad_header'
    huge = ref.SIGNATURE + ref.chunk(b'IHDR', struct.pack('>IIBBBBB', 40000, 40000, 8, 2, 0, 0, 0)) + ref.chunk(b'IDAT', b'x') + ref.chunk(b'IEND', b'')
    assert reason(huge) == 'too_large'
    assert reason(good, mode='index') == 'not_indexed'


def test_a_flipped_bit_in_any_chunks_crc_is_caught():
    from sniper_amd.png_decode import parse_png
    rng = np.random.default_rng(3)
    data = ref.png_bytes(9, 4, 8, 3, ref.random_rows(rng, 4, 9, 8, 3), palette=ref.palette_for(rng, 8), idat_split=11,
                         before_idat=[(b'gAMA', struct.pack('>I', 45455)), (b'tRNS', b'\0\1')], after_idat=[(b'tEXt', b'k\0v')])
    assert 'fallback' not in parse_png(data)
    pos, n_chunks = 8, 0
    while pos < len(data):
        n = struct.unpack('>I', data[pos:pos + 4])[0]
        crc_at = pos + 8 + n
        for bit in (0, 13, 31):
            bad = bytearray(data)
            bad[crc_at + bit // 8] ^= 1 << (bit % 8)
            assert parse_png(bytes(bad)) == {'fallback': 'bad_crc'}, (pos, bit)
        if n:          # ... and a flipped bit of the chunk's data
            bad = bytearray(data)
            bad[pos + 8] ^= 4
            assert parse_png(bytes(bad)) == {'fallback': 'bad_crc'}, pos
        pos += 12 + n
        n_chunks += 1
    assert n_chunks >= 8


# ---- the decoder of inflate_code.h as a host program -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp('inflate')
    return ref.compile_inflate_program(d), ref.compile_inflate_program(d, sanitize=True)


@pytest.fixture(scope='module')
def streams():
    return ref.stream_set()


def test_host_program_equals_zlib_on_the_stream_set(programs, streams):
    for exe in programs:
        # exact capacities, and capacities with room to spare
        for slack in (0, 5):
            got = ref.run_inflate_program(exe, [(s, len(d) + slack) for _, s, d in streams])
            for (name, s, d), (status, n, guard, out) in zip(streams, got):
                assert zlib.decompress(s) == d, name
                assert status == 0 and n == len(d) and guard and out == d, (name, status, n)


def test_every_damaged_stream_gives_exactly_its_status_bit_and_stays_inside_its_capacity(programs):
    damaged = ref.damaged_set()
    assert {bit for _, _, _, bit in damaged} == {1, 2, 4, 8, 16, 32, 64, 128, 256, 512}
    for exe in programs:
        got = ref.run_inflate_program(exe, [(s, cap) for _, s, cap, _ in damaged])
        for (name, s, cap, bit), (status, n, guard, out) in zip(damaged, got):
            assert status == bit, (name, status, bit)
            assert guard and n <= cap and len(out) == n, (name, n, cap)
    # what zlib itself says: it refuses every one but those that only the capacity or the bytes behind the stream stop here
    for name, s, cap, bit in damaged:
        if bit in (128, 512):
            zlib.decompressobj().decompress(s)
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(s)


def test_every_truncation_and_every_flipped_byte_of_a_stream_ends_with_a_status_inside_the_capacity(programs, streams):
    # bounded by construction: whatever the bytes, the decoder ends, reads nothing past the stream (the sanitizer build's heap
    # block is exactly the stream) and stores nothing past the capacity
    rng = np.random.default_rng(9)
    pick = {n: (s, d) for n, s, d in streams}
    cases = []
    for name in ('dynamic', 'fixed', 'cross_repeat', 'deep_code', 'two_blocks', 'single_distance'):
        s, d = pick[name]
        for cut in range(0, len(s), max(1, len(s) // 40)):
            cases.append((s[:cut], len(d)))
        for _ in range(60):
            b = bytearray(s)
            b[int(rng.integers(2, len(s)))] ^= 1 << int(rng.integers(0, 8))
            cases.append((bytes(b), len(d) + 7))
    got = ref.run_inflate_program(programs[1], cases)
    for (s, cap), (status, n, guard, out) in zip(cases, got):
        assert guard and n <= cap
        assert status in (0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512), status
        try:
            want = zlib.decompress(s)
        except zlib.error:
            assert status != 0 or len(s) == 0
        else:
            assert status in (0, 128) and (status or out == want)


def test_census_of_the_stream_set(streams):
    total = {}
    sizes = []
    for name, s, d in streams:
        out, info = ref.trace_inflate(s)
        assert out == d, name
        sizes.append(len(d))
        for k, v in info.items():
            if isinstance(v, set):
                total.setdefault(k, set()).update(v)
            elif isinstance(v, bool) or isinstance(v, np.bool_):
                total[k] = bool(total.get(k, False) or v)
            elif k == 'max_code':
                total[k] = max(total.get(k, 0), v)
            else:
                total[k] = total.get(k, 0) + int(v)
        if name == 'flushes':
            assert info['blocks'] >= 4 and info['empty_stored'] >= 2          # several blocks, Z_FULL_FLUSH's empty stored blocks
    assert total['types'] == {0, 1, 2}
    assert total['empty_stored'] >= 3
    assert total['len_syms'] == set(range(257, 286)) and total['dist_syms'] == set(range(30))
    assert total['rep_syms'] == {16, 17, 18} and total['cross_repeat']
    assert total['max_code'] == 15
    assert total['no_dist_block'] and total['single_dist_block']
    assert total['overlap'] and total['d1_l258'] and total['dist_32768']
    assert total['prev_block'] and total['straddle']
    assert {0, 1, 32767, 32768, 32769, 65537} <= set(sizes)


# ---- parse_inst ------------------------------------------------------------------------------------------------------------------
def test_parse_inst_restatement_on_hand_made_maps():
    obj = np.array([[0, 1, 1, 0],
                    [2, 1, 0, 0],
                    [2, 0, 0, 255]], np.uint8)
    cls = np.array([[0, 5, 5, 0],
                    [9, 5, 0, 0],
                    [9, 0, 0, 255]], np.uint8)
    rec = ref.parse_inst_ref(obj, cls)
    assert [int(r['mask_cls']) for r in rec] == [5, 9, 255]
    assert [r['mask_bound'].tolist() for r in rec] == [[1, 0, 2, 1], [0, 1, 0, 2], [3, 2, 3, 2]]
    assert rec[0]['mask'].tolist() == [[True, True], [True, False]] and rec[1]['mask'].tolist() == [[True], [True]]
    assert rec[0]['mask'].dtype == np.bool_ and rec[0]['mask_bound'].dtype == np.dtype(int)
    cls[1, 1] = 6
    with pytest.raises(AssertionError):
        ref.parse_inst_ref(obj, cls)
    for o, c in ref.voc_maps():
        rec = ref.parse_inst_ref(o, c)
        assert [k for k in np.unique(o) if k] == [int(o[r['mask_bound'][1]:r['mask_bound'][3] + 1, r['mask_bound'][0]:r['mask_bound'][2] + 1][r['mask']][0])
                                                  for r in rec]
    big = ref.voc_maps()[2]
    assert big[0].shape == (375, 500) and 255 in big[0] and (big[0] == 7).sum() == 1
    assert ref.parse_inst_ref(*big)[2]['mask_bound'].tolist() == [0, 0, 499, 374]


def test_the_cache_keeps_pil_as_its_default(monkeypatch):
    from sniper_amd.data import im_worker as iw
    from sniper_amd.png_decode import is_png_path
    monkeypatch.delenv('SNIPER_IMAGE_DECODER', raising=False)
    assert iw.DeviceImageCache().decoder == 'pil'
    assert is_png_path('a/b.PNG') and is_png_path('x.png') and not is_png_path('x.png.jpg') and not is_png_path(np.zeros(3))
