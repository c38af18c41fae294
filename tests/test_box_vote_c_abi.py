"""CPU: sn_box_vote and sn_box_vote_limits are exported with their prototypes, and every argument sn_box_vote refuses is refused by
name before any launch (NULL stream, no device: the pointers are never dereferenced)."""
import ctypes

import pytest

from test_c_abi import lib  # noqa: F401  (the module-scoped fixture that builds and loads the library)


def _call(lib, P=3, n_tiles=3, thresh=0.8, method=0, null=None, ptrs=None):  # noqa: F811
    args = list(ptrs or [ctypes.c_void_p(1024 * (k + 1)) for k in range(5)])
    if null is not None:
        args[null] = None
    return lib.call('sn_box_vote', *args, n_tiles, P, thresh, method, None)


def test_entry_points_are_exported_with_their_prototypes(lib):  # noqa: F811
    ret, argtypes, names = lib.protos['sn_box_vote']
    assert names == ['d_top_rows', 'd_all_rows', 'd_off', 'd_top_count', 'd_tiles', 'n_tiles', 'P', 'thresh', 'method', 'stream']
    assert ret is ctypes.c_int
    assert argtypes == [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    assert hasattr(lib.raw('sn_box_vote'), 'argtypes')
    ret, argtypes, names = lib.protos['sn_box_vote_limits']
    assert names == ['h_out2'] and ret is ctypes.c_int and argtypes == [ctypes.c_void_p]


def test_limits_need_no_device(lib):  # noqa: F811
    from sniper_amd.ext import box_vote
    lim = box_vote.limits()
    assert lim == {'tile': 64, 'chunk': 128}             # one kept row per lane of a wave; 128 rows of 5 doubles = 5 KB of LDS
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call('sn_box_vote_limits', None)
    assert 'sn_box_vote_limits' in str(e.value) and 'null pointer' in str(e.value)


def test_nothing_to_do_is_no_launch(lib):  # noqa: F811
    assert _call(lib, P=0) == 0                           # (the pointers are not dereferenced and no device is needed)
    assert _call(lib, P=4, n_tiles=0) == 0


def _misaligned(k):
    p = [ctypes.c_void_p(1024 * (j + 1)) for j in range(5)]
    p[k] = ctypes.c_void_p(1024 * (k + 1) + 2)
    return p


@pytest.mark.parametrize('kw,words', [
    (dict(null=0), ('null pointer',)),
    (dict(null=1), ('null pointer',)),
    (dict(null=2), ('null pointer',)),
    (dict(null=3), ('null pointer',)),
    (dict(null=4), ('null pointer',)),
    (dict(P=-1), ('P >= 0', 'P = -1')),
    (dict(n_tiles=-2), ('n_tiles >= 0', 'n_tiles = -2')),
    (dict(thresh=0.0), ('thresh in (0, 1]', 'thresh = 0')),
    (dict(thresh=-0.5), ('thresh in (0, 1]', 'thresh = -0.5')),
    (dict(thresh=1.5), ('thresh in (0, 1]', 'thresh = 1.5')),
    (dict(thresh=float('nan')), ('thresh in (0, 1]', 'nan')),
    (dict(method=3), ('unknown method 3',)),
    (dict(method=-1), ('unknown method -1',)),
    (dict(ptrs=_misaligned(0)), ('misaligned',)),
    (dict(ptrs=_misaligned(1)), ('misaligned',)),
    (dict(ptrs=_misaligned(2)), ('misaligned',)),
    (dict(ptrs=_misaligned(3)), ('misaligned',)),
    (dict(ptrs=_misaligned(4)), ('misaligned',)),
    (dict(ptrs=[ctypes.c_void_p(1024)] * 2 + [ctypes.c_void_p(4096)] * 3), ('d_top_rows aliases d_all_rows',)),
    (dict(P=0, thresh=2.0), ('thresh in (0, 1]',)),        # refused even when there is nothing to do
])
def test_refused_arguments(lib, kw, words):  # noqa: F811
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        _call(lib, **kw)
    msg = str(e.value)
    assert 'sn_box_vote' in msg and all(w in msg for w in words), msg
