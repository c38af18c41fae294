"""CPU: every argument error of sn_render_dets / sn_render_limits is reported before any launch, by a message that names the function
and the condition (the device pointers are not dereferenced: there is no GPU here, a launch would fail with another message)."""
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
ALWAYS = ('src', 'hw', 'pix_off', 'item_off', 'out')
ITEMS = ('rects', 'colors', 'mask_idx', 'text_off')


def _call(form=0, I=2, max_h=48, max_w=64, pixels=4000, max_items=10, items=15, h_text=None, n_text=40, G=8, gh=7, gw=5, n_masks=3, M=28,
          thr=0.4, alpha=102, lw=3, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_render_dets', form, g('src'), g('hw'), g('pix_off'), I, max_h, max_w, pixels, g('item_off'), max_items, items, g('rects'),
            g('colors'), g('mask_idx'), g('text_off'), g('text'), h_text, n_text, g('atlas'), G, gh, gw, g('masks'), n_masks, M, thr, alpha, lw,
            0.0, 0.0, 0.0, g('out'), None)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert (call[0] + ':') in msg and all(w in msg for w in words), msg


def test_limits(lib):
    out = (ctypes.c_int32 * 5)()
    assert lib.call('sn_render_limits', out) == 0
    max_items, tw, th, per_round, threads = list(out)
    assert max_items >= 1024 and per_round >= 64 and per_round % 64 == 0 and threads % 64 == 0
    assert tw == 64 and th % (threads // 64) == 0           # a lane per column, whole rows per wave
    _refused(lib, ('null pointer',), ('sn_render_limits', None))


def test_null_pointers(lib):
    for name in ALWAYS:
        _refused(lib, ('null pointer',), _call(**{name: None}))
    for name in ITEMS:
        _refused(lib, ('null pointer', 'when there are items'), _call(**{name: None}))
    for name in ('text', 'atlas'):
        _refused(lib, ('null pointer', 'when there are glyphs'), _call(**{name: None}))
    _refused(lib, ('null pointer', 'masks'), _call(masks=None))


def test_conditions(lib):
    _refused(lib, ('form', 'form = 2'), _call(form=2))
    _refused(lib, ('1 <= I', 'I = 0'), _call(I=0))
    _refused(lib, ('1 <= I', 'I = 65536'), _call(I=65536))
    lim = (ctypes.c_int32 * 5)()
    lib.call('sn_render_limits', lim)
    _refused(lib, ('an image has %d items' % (lim[0] + 1), 'at most %d' % lim[0]), _call(max_items=lim[0] + 1))
    _refused(lib, ('1 <= M <= 1024', 'M = 0'), _call(M=0))
    _refused(lib, ('1 <= M <= 1024', 'M = 1025'), _call(M=1025))
    _refused(lib, ('n_masks * M * M < 2^31',), _call(n_masks=4096, M=1024))
    _refused(lib, ('0 <= mask_alpha <= 256', 'mask_alpha = -1'), _call(alpha=-1))
    _refused(lib, ('0 <= mask_alpha <= 256', 'mask_alpha = 257'), _call(alpha=257))
    _refused(lib, ('1 <= line_width', 'line_width = 0'), _call(lw=0))
    _refused(lib, ('h * w < 2^31', 'max_h = 65536', 'max_w = 32768'), _call(max_h=65536, max_w=32768))
    _refused(lib, ('h >= 1', 'max_h = 0'), _call(max_h=0))
    _refused(lib, ('total_pixels < 2^40', 'total_pixels = 1099511627776'), _call(pixels=1 << 40))
    _refused(lib, ('total_pixels', 'total_pixels = 1'), _call(pixels=1))
    _refused(lib, ('32-bit indexing', 'total_items = 536870912'), _call(items=1 << 29))
    _refused(lib, ('32-bit indexing', 'total_items = -1'), _call(items=-1))
    _refused(lib, ('32-bit indexing', 'total_text = 4194304'), _call(n_text=1 << 22))
    _refused(lib, ('atlas', 'G = 0'), _call(G=0))
    _refused(lib, ('atlas', 'gw = 257'), _call(gw=257))


def test_glyph_indices_are_checked_where_the_host_sees_them(lib):
    text = np.array([0, 7, 3, 8, 1], np.int32)
    _refused(lib, ('glyph index 8', 'position 3', 'G = 8'), _call(h_text=ctypes.c_void_p(text.ctypes.data), n_text=5))
    text[3] = -1
    _refused(lib, ('glyph index -1', 'position 3'), _call(h_text=ctypes.c_void_p(text.ctypes.data), n_text=5))


def test_header_and_library_export_the_render_entry_points(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_')}
    assert {'sn_render_limits', 'sn_render_dets'} <= exported and {'sn_render_limits', 'sn_render_dets'} <= set(lib.protos)
