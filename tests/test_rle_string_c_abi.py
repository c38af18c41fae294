"""CPU: every argument error of the sn_rle_string_* / sn_rle_to_string / sn_rle_from_string entry points is reported before any launch,
by a message that names the function and the condition (device pointers are not dereferenced: there is no GPU here, a launch would
fail with another message; the HOST copies of the offsets are real arrays, they are what the entry points check)."""
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
OK3 = np.array([0, 2, 5, 9], np.int32)             # N = 3, total 9
NAMES = ('sn_rle_string_len', 'sn_rle_to_string', 'sn_rle_string_count', 'sn_rle_from_string')


def _h(a):
    return ctypes.c_void_p(a.ctypes.data)


def _call(name, N=3, n_runs=9, n_chars=9, h_run=OK3, h_str=OK3, **ptr):
    g = lambda k: ptr.get(k, P)
    hr, hs = (None if 'h_run_off' in ptr else _h(h_run)), (None if 'h_str_off' in ptr else _h(h_str))
    if name == 'sn_rle_string_len':
        return (name, g('cnts'), g('run_off'), hr, N, n_runs, g('str_len'), None)
    if name == 'sn_rle_to_string':
        return (name, g('cnts'), g('run_off'), hr, g('str_off'), hs, N, n_runs, n_chars, g('chars'), None)
    if name == 'sn_rle_string_count':
        return (name, g('chars'), g('str_off'), hs, N, n_chars, g('m'), g('status'), None)
    return (name, g('chars'), g('str_off'), hs, g('run_off'), hr, g('status'), N, n_chars, n_runs, g('cnts'), None)


PTRS = {'sn_rle_string_len': ('cnts', 'run_off', 'h_run_off', 'str_len'),
        'sn_rle_to_string': ('cnts', 'run_off', 'h_run_off', 'str_off', 'h_str_off', 'chars'),
        'sn_rle_string_count': ('chars', 'str_off', 'h_str_off', 'm', 'status'),
        'sn_rle_from_string': ('chars', 'str_off', 'h_str_off', 'run_off', 'h_run_off', 'status', 'cnts')}


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert call[0] + ':' in msg and all(w in msg for w in words), msg


def test_limits(lib):
    from sniper_amd.results import rle_string_limits
    out = (ctypes.c_int32 * 3)()
    assert lib.call('sn_rle_string_limits', out) == 0
    threads, chunk, max_chars = list(out)
    assert threads % 64 == 0 and chunk >= 64 and max_chars == 7            # 5 * 7 = 35 bits: any difference of two uint32 counts
    assert rle_string_limits() == {'threads': threads, 'chunk': chunk, 'max_chars': max_chars}
    _refused(lib, ('null pointer',), ('sn_rle_string_limits', None))
    box = (ctypes.c_int32 * 5)()
    lib.call('sn_rle_limits', box)                                        # the older query is what it was
    assert list(box) == [1024, 256, 64, 4, 256]


def test_null_pointers(lib):
    for name in NAMES:
        for p in PTRS[name]:
            _refused(lib, ('null pointer',), _call(name, **{p: None}))


def test_counts_and_totals(lib):
    for name in NAMES:
        _refused(lib, ('1 <= N', 'N = 0'), _call(name, N=0))
        _refused(lib, ('1 <= N', 'N = -3'), _call(name, N=-3))
        _refused(lib, ('1 <= N', 'N = 2147483647'), _call(name, N=2 ** 31 - 1))
    for name in ('sn_rle_string_len', 'sn_rle_to_string', 'sn_rle_from_string'):
        _refused(lib, ('32-bit indexing', 'total_runs = 2147483648'), _call(name, n_runs=2 ** 31))
        _refused(lib, ('32-bit indexing', 'total_runs = -1'), _call(name, n_runs=-1))
    for name in ('sn_rle_to_string', 'sn_rle_string_count', 'sn_rle_from_string'):
        _refused(lib, ('32-bit indexing', 'total_chars = 2147483648'), _call(name, n_chars=2 ** 31))
        _refused(lib, ('32-bit indexing', 'total_chars = -1'), _call(name, n_chars=-1))


def test_offsets(lib):
    late, down, short = np.array([1, 2, 5, 9], np.int32), np.array([0, 5, 2, 9], np.int32), np.array([0, 2, 5, 8], np.int32)
    for name in NAMES:
        for key, label in (('h_run', 'run_off'), ('h_str', 'str_off')):
            if ('h_%s' % label) not in PTRS[name]:
                continue
            _refused(lib, ('the offsets ' + label, 'do not start at 0'), _call(name, **{key: late}))
            _refused(lib, ('the offsets ' + label, 'decrease'), _call(name, **{key: down}))
            _refused(lib, ('the offsets ' + label, 'do not end at the total given', 'total = 9'), _call(name, **{key: short}))


def test_header_and_library_export_the_same_symbols(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    mine = lambda n: n.startswith('sn_rle_string_') or n in ('sn_rle_to_string', 'sn_rle_from_string')
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and mine(ln.split()[-1])}
    declared = {n for n in lib.protos if mine(n)}
    assert exported == declared == {'sn_rle_string_limits', 'sn_rle_string_len', 'sn_rle_to_string', 'sn_rle_string_count',
                                    'sn_rle_from_string'}
