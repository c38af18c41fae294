"""CPU: every argument error of the sn_inflate / sn_png_unfilter / sn_png_expand / sn_voc_inst_* entry points is reported before any
launch, by a message that names the function and the condition (the device pointers are not dereferenced: there is no GPU here),
and what the header declares is what the library exports."""
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
NAMES = {'sn_inflate_limits', 'sn_inflate', 'sn_png_unfilter', 'sn_png_expand', 'sn_vocgt_scan', 'sn_vocgt_crop'}


def _h(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    return a, ctypes.c_void_p(a.ctypes.data)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert (call[0] + ':') in msg and all(w in msg for w in words), msg


def _inflate(rows, S=None, total_in=100, out_total=1000, **ptr):
    keep, hp = _h(rows, np.int64)
    g = lambda k: ptr.get(k, P)
    return keep, ('sn_inflate', g('data'), total_in, g('tab'), ptr.get('h_tab', hp), len(keep) if S is None else S, g('out'), out_total,
                  g('meta'), None)


def _img(w=5, h=4, depth=8, ctype=2, row=None, bpp=None, plen=0):
    ch = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}.get(ctype, 1)
    return [w, h, depth, ctype, (w * ch * depth + 7) // 8 if row is None else row, max(1, ch * depth // 8) if bpp is None else bpp, plen, 0]


def _unfilter(imgs, offs, I=None, raw_total=10000, **ptr):
    keep = (_h(imgs, np.int32), _h(offs, np.int64))
    g = lambda k: ptr.get(k, P)
    return keep, ('sn_png_unfilter', g('raw'), raw_total, g('img'), ptr.get('h_img', keep[0][1]), g('raw_off'), ptr.get('h_raw_off', keep[1][1]),
                  len(imgs) if I is None else I, g('meta'), None)


def _expand(imgs, offs, I=None, raw_total=10000, mode=0, **ptr):
    keep = (_h(imgs, np.int32), _h(offs, np.int64))
    g = lambda k: ptr.get(k, P)
    return keep, ('sn_png_expand', g('raw'), raw_total, g('img'), ptr.get('h_img', keep[0][1]), g('raw_off'), ptr.get('h_raw_off', keep[1][1]),
                  len(imgs) if I is None else I, g('pal'), g('out_ptrs'), g('meta'), mode, None)


def test_limits(lib):
    out = (ctypes.c_int32 * 6)()
    assert lib.call('sn_inflate_limits', out) == 0
    max_streams, max_bytes, lds, window, lanes, flush = list(out)
    assert max_streams == 65535 and max_bytes == 1 << 30 and window == 32768 and lanes == 64
    assert window < lds <= 40 * 1024 and flush + 258 + 256 <= window
    _refused(lib, ('null pointer',), ('sn_inflate_limits', None))


def test_inflate_conditions(lib):
    tab = [[0, 40, 0, 500], [40, 60, 512, 488]]
    for name in ('data', 'tab', 'h_tab', 'out', 'meta'):
        _refused(lib, ('null pointer',), _inflate(tab, **{name: None})[1])
    _refused(lib, ('1 <= S <= 65535', 'S = 0'), _inflate(tab, S=0)[1])
    _refused(lib, ('1 <= S <= 65535', 'S = 65536'), _inflate(tab, S=65536)[1])
    _refused(lib, ('total_in = -1',), _inflate(tab, total_in=-1)[1])
    _refused(lib, ('out_total = -5',), _inflate(tab, out_total=-5)[1])
    _refused(lib, ('stream 1 lies at 40 + 61', 'total_in = 100'), _inflate([[0, 40, 0, 500], [40, 61, 512, 488]])[1])
    _refused(lib, ('stream 0 lies at -1 + 4',), _inflate([[-1, 4, 0, 500]])[1])
    _refused(lib, ('the output of stream 1 lies at 499 + 10', 'behind the output before it'), _inflate([[0, 40, 0, 500], [40, 60, 499, 10]])[1])
    _refused(lib, ('the output of stream 1 lies at 512 + 489', 'out_total = 1000'), _inflate([[0, 40, 0, 500], [40, 60, 512, 489]])[1])
    _refused(lib, ('the output of stream 0 lies at 0 + -3',), _inflate([[0, 40, 0, -3]])[1])


@pytest.mark.parametrize('make', [_unfilter, _expand], ids=['unfilter', 'expand'])
def test_image_conditions(lib, make):
    fn = 'sn_png_unfilter' if make is _unfilter else 'sn_png_expand'
    good = [_img(), _img(13, 9, 2, 3, plen=4)]
    offs = [0, 64]
    names = ('raw', 'img', 'h_img', 'raw_off', 'h_raw_off', 'meta') + (() if make is _unfilter else ('pal', 'out_ptrs'))
    for name in names:
        _refused(lib, ('null pointer',), make(good, offs, **{name: None})[1])
    _refused(lib, ('1 <= I <= 65535', 'I = 0'), make(good, offs, I=0)[1])
    _refused(lib, ('raw_total = -1',), make(good, offs, raw_total=-1)[1])
    _refused(lib, ('image 1', '1 <= w, h'), make([_img(), _img(0, 3)], offs)[1])
    _refused(lib, ('image 0', 'w * h < 2^29'), make([_img(1 << 15, 1 << 15)], [0], raw_total=1 << 39)[1])
    _refused(lib, ('image 0', 'colour type'), make([_img(ctype=5)], [0])[1])
    _refused(lib, ('image 0', 'bit depth'), make([_img(depth=16, ctype=0)], [0])[1])
    _refused(lib, ('image 0', 'bit depth'), make([_img(depth=4, ctype=2)], [0])[1])
    _refused(lib, ('image 1', 'row bytes'), make([_img(), _img(row=14)], offs)[1])
    _refused(lib, ('image 0', 'bpp'), make([_img(bpp=4)], [0])[1])
    _refused(lib, ('image 0', 'palette entries'), make([_img(ctype=3, plen=257)], [0])[1])
    _refused(lib, ('image 1', 'overlap or pass raw_total'), make(good, [0, 63])[1])
    _refused(lib, ('image 1', 'overlap or pass raw_total'), make(good, offs, raw_total=64 + 9 * 5 - 1)[1])


def test_expand_modes(lib):
    _refused(lib, ('mode 0 (BGR) or 1 (indices)', 'mode = 2'), _expand([_img()], [0], mode=2)[1])
    _refused(lib, ('image 0', 'index mode takes grey and palette'), _expand([_img()], [0], mode=1)[1])


def test_voc_conditions(lib):
    hw, hp = _h([[4, 5], [3, 3]], np.int32)
    scan = lambda **k: ('sn_vocgt_scan', k.get('obj', P), k.get('cls', P), k.get('hw', P), k.get('h_hw', hp), k.get('I', 2), k.get('inst', P), None)
    for name in ('obj', 'cls', 'hw', 'h_hw', 'inst'):
        _refused(lib, ('null pointer',), scan(**{name: None}))
    _refused(lib, ('1 <= I <= 65535', 'I = 0'), scan(I=0))
    bad, bp = _h([[4, 0]], np.int32)
    _refused(lib, ('h >= 1, w >= 1',), scan(h_hw=bp, I=1))

    def crop(rows, off, N=None, total=None, **k):
        keep = (_h(rows, np.int32), _h(off, np.int64))
        g = lambda n: k.get(n, P)
        return keep, ('sn_vocgt_crop', g('obj'), g('hw'), k.get('h_hw', hp), k.get('I', 2), g('rec'), k.get('h_rec', keep[0][1]), g('pool_off'),
                      k.get('h_pool_off', keep[1][1]), len(rows) if N is None else N, g('pool'), off[-1] if total is None else total, None)
    rec, off = [[0, 1, 1, 1, 3, 2], [1, 255, 0, 0, 3, 3]], [0, 6, 15]
    for name in ('obj', 'hw', 'h_hw', 'rec', 'h_rec', 'pool_off', 'h_pool_off', 'pool'):
        _refused(lib, ('null pointer',), crop(rec, off, **{name: None})[1])
    _refused(lib, ('1 <= N <= 65535', 'N = 0'), crop(rec, off, N=0)[1])
    _refused(lib, ('record 1 names image 2',), crop([rec[0], [2, 1, 0, 0, 1, 1]], [0, 6, 7])[1])
    _refused(lib, ('record 0 names image 0 and id 0',), crop([[0, 0, 0, 0, 1, 1]], [0, 1])[1])
    _refused(lib, ('the bound of record 0', 'leaves its 4 x 5 map'), crop([[0, 1, 3, 1, 3, 2]], [0, 6])[1])
    _refused(lib, ('pool_off[1] = 7', 'give 6'), crop(rec, [0, 7, 16])[1])
    _refused(lib, ('pool_total = 14',), crop(rec, off, total=14)[1])


def test_header_and_library_export_the_new_entry_points(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_')}
    assert NAMES <= exported and NAMES <= set(lib.protos)
    assert exported == set(lib.protos)                    # declared = exported, the whole library
