"""CPU: every argument error of the sn_gdeform_* entry points is reported before any launch, by a message that names the
condition (the pointers are not dereferenced: there is no GPU here, a launch would fail with another message)."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


P = ctypes.c_void_p(16)
WS = 1 << 30


def _fwd(x=P, off=P, w=P, y=P, N=1, H=8, W=8, C=64, xps=None, O=64, yps=None, groups=2, dg=2, KH=3, KW=3, stride=1, pad=1, dil=1,
         ops=None, odt=0):
    return ('sn_gdeform_fwd', x, off, w, None, y, N, H, W, C, C if xps is None else xps, O, O if yps is None else yps, groups, dg, KH, KW,
            stride, pad, dil, 18 * dg if ops is None else ops, odt, 0, None)


def _dcol(dy=P, w=P, dcol=P, N=1, H=8, W=8, C=64, O=64, yps=None, groups=2, dg=2, KH=3, KW=3, stride=1, pad=1, dil=1, **_):
    return ('sn_gdeform_dcol', dy, w, dcol, N, H, W, C, O, O if yps is None else yps, groups, KH, KW, stride, pad, dil, None)


def _wgrad(dy=P, x=P, off=P, dw=P, N=1, H=8, W=8, C=64, O=64, yps=None, xps=None, groups=2, dg=2, KH=3, KW=3, stride=1, pad=1, dil=1,
           ops=None, odt=0, ws=P, ws_bytes=WS):
    return ('sn_gdeform_wgrad', dy, x, off, dw, N, H, W, C, O, O if yps is None else yps, C if xps is None else xps, groups, dg, KH, KW,
            stride, pad, dil, 18 * dg if ops is None else ops, odt, ws, ws_bytes, None)


ALL = (_fwd, _dcol, _wgrad)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert call[0] in msg and all(w in msg for w in words), msg


def test_null_pointers(lib):
    for kw in (dict(x=None), dict(off=None), dict(w=None), dict(y=None)):
        _refused(lib, ('null pointer',), _fwd(**kw))
    for kw in (dict(dy=None), dict(w=None), dict(dcol=None)):
        _refused(lib, ('null pointer',), _dcol(**kw))
    for kw in (dict(dy=None), dict(x=None), dict(off=None), dict(dw=None)):
        _refused(lib, ('null pointer',), _wgrad(**kw))


@pytest.mark.parametrize('make', ALL)
def test_shape_conditions(lib, make):
    _refused(lib, ('groups == 1', 'dense'), make(groups=1, dg=1))
    _refused(lib, ('Cg != Og',), make(C=64, O=128, groups=2))
    _refused(lib, ('slab grid', 'C = 48'), make(C=48, O=48, groups=3, dg=1))          # Cg = 16, C % 32 != 0
    _refused(lib, ('slab grid', 'C / groups = 2'), make(C=64, O=64, groups=32))
    _refused(lib, ('slab grid', 'C / groups = 64'), make(C=128, O=128, groups=2))
    _refused(lib, ('5x5', 'only 3x3'), make(KH=5, KW=5, pad=2))
    _refused(lib, ('1x1', 'only 3x3'), make(KH=1, KW=1, pad=0))
    _refused(lib, ('bad geometry',), make(stride=0))
    _refused(lib, ('too many pixels', '32-bit'), make(H=16384, W=16384))
    _refused(lib, ('pixel pitches',), make(yps=60))


@pytest.mark.parametrize('make', (_fwd, _wgrad))
def test_offset_conditions(lib, make):
    _refused(lib, ('deformable group splits a slab', '64 / 4'), make(C=64, dg=4))
    _refused(lib, ('deformable group splits a slab',), make(C=96, O=96, groups=6, dg=2))     # 48 channels per deformable group
    _refused(lib, ('bad geometry',), make(dg=0))
    _refused(lib, ('offset_dtype',), make(odt=2))
    _refused(lib, ('offset_pix_stride',), make(ops=18))
    _refused(lib, ('pixel pitches',), make(xps=32))


def test_column_index_overflow(lib):
    # 2^23 pixels pass the pixel limit; 2^23 * 9 * 64 column elements do not fit 32-bit indexing
    _refused(lib, ('too many column elements', '32-bit'), _dcol(H=2048, W=4096))


def test_short_workspace(lib):
    raw = lib.raw('sn_gdeform_wgrad_workspace_bytes')
    raw.restype = ctypes.c_size_t
    need = raw(2, 13, 11, 64, 64, 2, 3, 3, 1, 1, 1)
    assert need >= 4 * 64 * 9 * 32                   # at least one block of partials, one float per weight
    _refused(lib, ('short workspace', 'sn_gdeform_wgrad_workspace_bytes'), _wgrad(N=2, H=13, W=11, ws_bytes=need // 2))
    _refused(lib, ('short workspace',), _wgrad(N=2, H=13, W=11, ws=None, ws_bytes=need))
    # shapes the entry point refuses need no workspace
    assert raw(2, 13, 11, 64, 64, 1, 3, 3, 1, 1, 1) == 0 and raw(2, 13, 11, 64, 64, 2, 5, 5, 1, 2, 1) == 0
