"""CPU: every argument error of the sn_jpeg_enc_* entry points is reported before any launch, by a message that names the function and
the condition (the device pointers are not dereferenced: there is no GPU here, a launch would fail with another message)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


P = ctypes.c_void_p(64)
FACTORS = {0: (1, 1), 1: (2, 1), 2: (2, 2)}


def _blocks_of(h, w, ncomp, sampling):
    hs, vs = FACTORS.get(sampling, (1, 1)) if ncomp == 3 else (1, 1)
    return -(-w // (8 * hs)) * -(-h // (8 * vs)) * (hs * vs + ncomp - 1)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call[1])
    msg = str(e.value)
    assert (call[1][0] + ':') in msg and all(w in msg for w in words), msg


def _tables(sizes, ncomp, sampling, pix_off, blk_off):
    hw = np.ascontiguousarray(sizes, np.int32).reshape(-1, 2)
    if pix_off is None:
        pix_off = np.concatenate([[0], np.cumsum(hw[:, 0].astype(np.int64) * hw[:, 1])])
    if blk_off is None:
        blk_off = np.concatenate([[0], np.cumsum([_blocks_of(int(h), int(w), ncomp, sampling) if h > 0 and w > 0 else 0 for h, w in hw])])
    return hw, np.ascontiguousarray(pix_off, np.int64), np.ascontiguousarray(blk_off, np.int64)


def _hp(a):
    return ctypes.c_void_p(a.ctypes.data)


def _blocks(sizes, ncomp=3, sampling=2, quality=75, I=None, pixels=None, n_blocks=None, pix_table=None, blk_table=None, **ptr):
    hw, po, bo = _tables(sizes, ncomp, sampling, pix_table, blk_table)
    g = lambda k, d=P: ptr.get(k, d)
    return (hw, po, bo), ('sn_jpeg_enc_blocks', g('pix'), int(po[-1]) if pixels is None else pixels, g('hw'), g('h_hw', _hp(hw)), g('pix_off'),
                          g('h_pix_off', _hp(po)), g('blk_off'), g('h_blk_off', _hp(bo)), len(hw) if I is None else I,
                          int(bo[-1]) if n_blocks is None else n_blocks, ncomp, sampling, quality, g('coef'), None)


def _size(sizes, ncomp=3, sampling=2, I=None, n_blocks=None, blk_table=None, **ptr):
    hw, po, bo = _tables(sizes, ncomp, sampling, None, blk_table)
    g = lambda k, d=P: ptr.get(k, d)
    return (hw, bo), ('sn_jpeg_enc_size', g('coef'), g('hw'), g('h_hw', _hp(hw)), g('blk_off'), g('h_blk_off', _hp(bo)), len(hw) if I is None else I,
                      int(bo[-1]) if n_blocks is None else n_blocks, ncomp, sampling, g('bits'), g('status'), None)


def _raw_bound(bo):
    return int(sum(-(-(int(n) * 208 + 1) // 64) * 64 for n in np.diff(bo)))


def _write(sizes, ncomp=3, sampling=2, I=None, n_blocks=None, blk_table=None, raw_capacity=None, **ptr):
    hw, po, bo = _tables(sizes, ncomp, sampling, None, blk_table)
    g = lambda k, d=P: ptr.get(k, d)
    return (hw, bo), ('sn_jpeg_enc_write', g('coef'), g('hw'), g('h_hw', _hp(hw)), g('blk_off'), g('h_blk_off', _hp(bo)), len(hw) if I is None else I,
                      int(bo[-1]) if n_blocks is None else n_blocks, ncomp, sampling, g('bit_excl'), g('pic_first_bit'), g('chunk_off'), g('raw'),
                      _raw_bound(bo) if raw_capacity is None else raw_capacity, g('status'), None)


def _stuff(n_chunks=10, phase=2, I=2, raw_capacity=None, capacity=None, **ptr):
    g = lambda k, d=P: ptr.get(k, d)
    return None, ('sn_jpeg_enc_stuff', g('raw'), 64 * n_chunks if raw_capacity is None else raw_capacity, g('chunk_off'), g('raw_len'), I, n_chunks,
                  phase, g('cnt'), g('out_pos'), g('out'), 128 * n_chunks if capacity is None else capacity, None)


SIZES = [[16, 16], [24, 50], [1, 1]]


def test_limits(lib):
    out = (ctypes.c_int32 * 8)()
    assert lib.call('sn_jpeg_enc_limits', out) == 0
    assert list(out)[:5] == [256, 65535, 1 << 22, 208, 64] and out[7] == 2
    _refused(lib, ('null pointer',), (None, ('sn_jpeg_enc_limits', None)))


def test_null_pointers(lib):
    for name in ('pix', 'hw', 'h_hw', 'pix_off', 'h_pix_off', 'blk_off', 'h_blk_off', 'coef'):
        _refused(lib, ('null pointer',), _blocks(SIZES, **{name: None}))
    for name in ('coef', 'hw', 'h_hw', 'blk_off', 'h_blk_off', 'bits', 'status'):
        _refused(lib, ('null pointer',), _size(SIZES, **{name: None}))
    for name in ('coef', 'hw', 'h_hw', 'blk_off', 'h_blk_off', 'bit_excl', 'pic_first_bit', 'chunk_off', 'raw', 'status'):
        _refused(lib, ('null pointer',), _write(SIZES, **{name: None}))
    for name in ('raw', 'chunk_off', 'raw_len'):
        _refused(lib, ('null pointer',), _stuff(**{name: None}))
    _refused(lib, ('null pointer', 'cnt'), _stuff(phase=1, cnt=None))
    _refused(lib, ('null pointer', 'out_pos'), _stuff(phase=2, out_pos=None))
    _refused(lib, ('null pointer', 'out'), _stuff(phase=2, out=None))


@pytest.mark.parametrize('make', [_blocks, _size, _write], ids=['blocks', 'size', 'write'])
def test_counts_sizes_codes_and_offsets(lib, make):
    _refused(lib, ('1 <= I <= 65535', 'I = 0'), make(SIZES, I=0))
    _refused(lib, ('1 <= I <= 65535', 'I = 65536'), make(SIZES, I=65536))
    _refused(lib, ('picture 1', '1 <= h, w <= 65535'), make([[16, 16], [0, 5]]))
    _refused(lib, ('picture 0', '1 <= h, w <= 65535'), make([[4, -1]]))
    _refused(lib, ('picture 2', '1 <= h, w <= 65535'), make([[4, 4], [4, 4], [65536, 4]]))
    _refused(lib, ('picture 0', '1 <= h, w <= 65535'), make([[4, 65536]]))
    _refused(lib, ('ncomp = 2',), make(SIZES, ncomp=2))
    _refused(lib, ('ncomp = 4',), make(SIZES, ncomp=4))
    _refused(lib, ('sampling = 3',), make(SIZES, sampling=3))
    _refused(lib, ('sampling = -1',), make(SIZES, sampling=-1))
    # 16 x 16, 24 x 50, 1 x 1 in 4:2:0: 6, 2 * 4 * 6 = 48 and 6 blocks
    _refused(lib, ('picture 1', 'blk_off'), make(SIZES, blk_table=[0, 5, 54, 60]))
    _refused(lib, ('picture 3', 'blk_off does not end'), make(SIZES, blk_table=[0, 6, 54, 61]))
    _refused(lib, ('n_blocks = 59', 'the sizes give 60'), make(SIZES, n_blocks=59))
    # the same sizes are other blocks in another sampling: the offsets of 4:2:0 do not fit 4:4:4
    _refused(lib, ('picture 1', 'blk_off'), make(SIZES, sampling=0, blk_table=[0, 6, 54, 60]))
    # one call takes 2^22 blocks
    _refused(lib, ('at most 4194304 blocks',), make([[65535, 65535]], sampling=0))


def test_blocks_quality_and_pixel_offsets(lib):
    _refused(lib, ('quality = 0', '1 .. 100'), _blocks(SIZES, quality=0))
    _refused(lib, ('quality = 101', '1 .. 100'), _blocks(SIZES, quality=101))
    _refused(lib, ('picture 0', 'pix_off'), _blocks(SIZES, pix_table=[1, 257, 1457, 1458]))
    _refused(lib, ('picture 2', 'pix_off'), _blocks(SIZES, pix_table=[0, 256, 1455, 1457]))
    _refused(lib, ('picture 3', 'pix_off does not end'), _blocks(SIZES, pix_table=[0, 256, 1456, 1458]))
    _refused(lib, ('total_pixels = 1456', 'the sizes give 1457'), _blocks(SIZES, pixels=1456))


def test_write_and_stuff_capacities(lib):
    bound = 64 * (-(-(6 * 208 + 1) // 64) + -(-(48 * 208 + 1) // 64) + -(-(6 * 208 + 1) // 64))
    _refused(lib, ('raw_capacity = %d' % (bound - 64), 'at least the bound %d' % bound), _write(SIZES, raw_capacity=bound - 64))
    _refused(lib, ('raw_capacity = %d' % (bound + 4), 'a multiple of 64'), _write(SIZES, raw_capacity=bound + 4))
    _refused(lib, ('phase = 0',), _stuff(phase=0))
    _refused(lib, ('phase = 3',), _stuff(phase=3))
    _refused(lib, ('1 <= I <= 65535', 'I = 0'), _stuff(I=0))
    _refused(lib, ('n_chunks = 0',), _stuff(n_chunks=0))
    _refused(lib, ('raw_capacity = 639', 'below n_chunks * 64 = 640'), _stuff(raw_capacity=639))
    _refused(lib, ('capacity = 1279', 'below the bound 1280'), _stuff(capacity=1279))


def test_header_and_library_export_the_jpeg_enc_entry_points(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_jpeg_enc')}
    names = {'sn_jpeg_enc_limits', 'sn_jpeg_enc_blocks', 'sn_jpeg_enc_size', 'sn_jpeg_enc_write', 'sn_jpeg_enc_stuff'}
    assert names == exported and names <= set(lib.protos)
