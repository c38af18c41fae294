"""CPU: every argument error of the sn_deflate_* / sn_png_filter entry points is reported before any launch, by a message that names the
function and the condition (the device pointers are not dereferenced: there is no GPU here, a launch would fail with another
message)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


P = ctypes.c_void_p(16)
B = 32768


def _h(a, dtype=np.int64):
    a = np.ascontiguousarray(a, dtype)
    return a, ctypes.c_void_p(a.ctypes.data)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert (call[0] + ':') in msg and all(w in msg for w in words), msg


def _plan(h_off, S=None, total=None, **ptr):
    keep, hp = _h(h_off)
    g = lambda k: ptr.get(k, P)
    S = len(h_off) - 1 if S is None else S
    return keep, ('sn_deflate_plan', g('offsets'), ptr.get('h_offsets', hp), S, int(h_off[-1]) if total is None else total, g('blk_first'), None)


def _code(h_off, S=None, total=None, n_blocks=None, **ptr):
    keep, hp = _h(h_off)
    g = lambda k: ptr.get(k, P)
    S = len(h_off) - 1 if S is None else S
    nb = sum(max(1, -(-(b - a) // B)) for a, b in zip(h_off, h_off[1:])) if n_blocks is None else n_blocks
    return keep, ('sn_deflate_code', g('data'), g('offsets'), ptr.get('h_offsets', hp), S, int(h_off[-1]) if total is None else total,
                  g('blk_first'), nb, g('blk_code'), g('blk_size'), None)


def _write(h_off, S=None, total=None, n_blocks=None, capacity=None, **ptr):
    keep, hp = _h(h_off)
    g = lambda k: ptr.get(k, P)
    S = len(h_off) - 1 if S is None else S
    sizes = [b - a for a, b in zip(h_off, h_off[1:])]
    nb = sum(max(1, -(-n // B)) for n in sizes) if n_blocks is None else n_blocks
    bound = sum(n + 5 * (-(-n // B) + 1) + 6 for n in sizes)
    return keep, ('sn_deflate_write', g('data'), g('offsets'), ptr.get('h_offsets', hp), S, int(h_off[-1]) if total is None else total,
                  g('blk_first'), nb, g('blk_code'), g('blk_pos'), g('out'), bound if capacity is None else capacity, None)


def _filter(sizes, I=None, pixels=None, stream=None, **ptr):
    keep, hp = _h(sizes, np.int32)
    g = lambda k: ptr.get(k, P)
    hw = np.asarray(sizes).reshape(-1, 2)
    return keep, ('sn_png_filter', g('pix'), g('hw'), ptr.get('h_hw', hp), g('pix_off'), g('stream_off'), len(hw) if I is None else I,
                  int((hw[:, 0] * hw[:, 1]).sum()) if pixels is None else pixels,
                  int((hw[:, 0] * (3 * hw[:, 1] + 1)).sum()) if stream is None else stream, g('out'), None)


def test_limits_and_bound(lib):
    out = (ctypes.c_int32 * 6)()
    assert lib.call('sn_deflate_limits', out) == 0
    block, threads, max_s, code_words, code_lds, write_lds = list(out)
    assert block == B and 8192 <= block <= 65535 and threads % 64 == 0 and max_s == 65535 and code_words > 286
    _refused(lib, ('null pointer',), ('sn_deflate_limits', None))
    bound = lib.raw('sn_deflate_bound')
    assert bound(0) == 11 and bound(1) == 17 and bound(B) == B + 16 and bound(B + 1) == B + 22 and bound(-1) == -1


def test_null_pointers(lib):
    off = [0, 10, 10, 40000]
    for name in ('offsets', 'h_offsets', 'blk_first'):
        _refused(lib, ('null pointer',), _plan(off, **{name: None})[1])
    for name in ('data', 'offsets', 'h_offsets', 'blk_first', 'blk_code', 'blk_size'):
        _refused(lib, ('null pointer',), _code(off, **{name: None})[1])
    for name in ('data', 'offsets', 'h_offsets', 'blk_first', 'blk_code', 'blk_pos', 'out'):
        _refused(lib, ('null pointer',), _write(off, **{name: None})[1])
    for name in ('pix', 'hw', 'h_hw', 'pix_off', 'stream_off', 'out'):
        _refused(lib, ('null pointer',), _filter([[4, 5]], **{name: None})[1])


@pytest.mark.parametrize('make', [_plan, _code, _write], ids=['plan', 'code', 'write'])
def test_stream_count_and_offsets(lib, make):
    _refused(lib, ('1 <= S <= 65535', 'S = 0'), make([0], S=0)[1])
    _refused(lib, ('1 <= S <= 65535', 'S = 65536'), make([0, 1], S=65536)[1])
    _refused(lib, ('offsets', 'do not start at 0'), make([1, 5])[1])
    _refused(lib, ('offsets', 'are not ascending'), make([0, 9, 5, 12])[1])
    _refused(lib, ('offsets', 'do not end at the total given', 'total = 13'), make([0, 9, 12], total=13)[1])
    _refused(lib, ('0 <= total < 2^40', 'total = -1'), make([0, 1], total=-1)[1])


def test_block_count_and_capacity(lib):
    off = [0, 10, 10, 10 + 2 * B + 1]              # 1 + 1 (empty) + 3 blocks
    _refused(lib, ('n_blocks = 4', 'give 5 blocks'), _code(off, n_blocks=4)[1])
    _refused(lib, ('n_blocks = 6', 'give 5 blocks'), _write(off, n_blocks=6)[1])
    bound = (10 + 16) + 11 + (2 * B + 1 + 5 * 4 + 6)
    _refused(lib, ('capacity = %d' % (bound - 1), 'below the bound %d' % bound), _write(off, capacity=bound - 1)[1])
    _refused(lib, ('capacity = 0', 'below the bound 11'), _write([0, 0], capacity=0)[1])


def test_filter_conditions(lib):
    _refused(lib, ('1 <= I <= 65535', 'I = 0'), _filter([[4, 5]], I=0)[1])
    _refused(lib, ('picture 1 is 0 x 5', 'h >= 1'), _filter([[4, 5], [0, 5]])[1])
    _refused(lib, ('picture 0 is 4 x -1', 'w >= 1'), _filter([[4, -1]])[1])
    _refused(lib, ('picture 0 is 32768 x 32768', 'h * w < 2^29'), _filter([[32768, 32768]])[1])
    _refused(lib, ('total_pixels = 21', 'the sizes give 20'), _filter([[4, 5]], pixels=21)[1])
    _refused(lib, ('total_stream = 60', 'the sizes give 64'), _filter([[4, 5]], stream=60)[1])


def test_header_and_library_export_the_png_entry_points(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_')}
    names = {'sn_deflate_limits', 'sn_deflate_bound', 'sn_deflate_plan', 'sn_deflate_code', 'sn_deflate_write', 'sn_png_filter'}
    assert names <= exported and names <= set(lib.protos)
