"""CPU: the sn_prop_* entry points exist with the declared signatures, and every argument error is reported before any launch, by a
message that names the function and the condition (the pointers are not dereferenced: there is no GPU here, a launch would fail
with another message)."""
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
NMS_PTRS = ('rows', 'off', 'keep', 'nkeep')
ASSIGN_PTRS = ('boxes', 'box_off', 'gt_box', 'gt_classes', 'gt_off', 'max_ov', 'max_cls', 'argmax')
RECALL_PTRS = ('boxes', 'box_off', 'gt_box', 'gt_mask', 'gt_off', 'thrs', 'gt_ov', 'num_pos', 'hits')


def _nms(I=3, max_n=50, total=120, thresh=0.7, ws=P, ws_bytes=WS, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_prop_nms', g('rows'), g('off'), I, max_n, total, thresh, ws, ws_bytes, g('keep'), g('nkeep'), None)


def _assign(I=3, max_n=50, max_g=20, total=120, NG=40, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_prop_assign', g('boxes'), g('box_off'), g('gt_box'), g('gt_classes'), g('gt_off'), I, max_n, max_g, total, NG, g('max_ov'),
            g('max_cls'), g('argmax'), None)


def _recall(I=3, A=7, T=10, max_g=20, total=120, NG=40, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_prop_recall', g('boxes'), g('box_off'), g('gt_box'), g('gt_mask'), g('gt_off'), g('thrs'), I, A, T, max_g, total, NG,
            g('gt_ov'), g('num_pos'), g('hits'), None)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert call[0] + ':' in msg and all(w in msg for w in words), msg


def _limits(lib):
    out = (ctypes.c_int32 * 6)()
    assert lib.call('sn_prop_limits', out) == 0
    return list(out)


def test_limits_admit_what_the_issue_asks(lib):
    max_gt, max_t, assign_block, recall_threads, nms_tile, sort_tile = _limits(lib)
    assert max_gt >= 256 and max_t >= 10 and assign_block >= 64 and recall_threads >= 64 and nms_tile == 64 and sort_tile >= 64
    assert max_gt % recall_threads == 0
    _refused(lib, ('null pointer',), ('sn_prop_limits', None))
    import re
    from sniper_amd._lib import HEADER
    with open(HEADER) as fh:
        defs = dict(re.findall(r'#define (SN_PROP_MAX_\w+) (\d+)', fh.read()))
    assert defs == {'SN_PROP_MAX_GT': str(max_gt), 'SN_PROP_MAX_T': str(max_t)}


def test_declared_signatures(lib):
    c = ctypes
    vp = c.c_void_p
    want = {
        'sn_prop_limits': (c.c_int, [vp]),
        'sn_prop_nms_workspace_bytes': (c.c_size_t, [c.c_long]),
        'sn_prop_nms': (c.c_int, [vp, vp, c.c_int, c.c_int, c.c_long, c.c_float, vp, c.c_size_t, vp, vp, vp]),
        'sn_prop_assign': (c.c_int, [vp] * 5 + [c.c_int, c.c_int, c.c_int, c.c_long, c.c_long, vp, vp, vp, vp]),
        'sn_prop_recall': (c.c_int, [vp] * 6 + [c.c_int, c.c_int, c.c_int, c.c_int, c.c_long, c.c_long, vp, vp, vp, vp]),
    }
    for name, (ret, args) in want.items():
        assert lib.protos[name][0] is ret and lib.protos[name][1] == args, name
        assert lib.protos[name][2][-1] == 'stream' or name in ('sn_prop_limits', 'sn_prop_nms_workspace_bytes')


def test_null_pointers(lib):
    for name in NMS_PTRS:
        _refused(lib, ('null pointer',), _nms(**{name: None}))
    for name in ASSIGN_PTRS:
        _refused(lib, ('null pointer',), _assign(**{name: None}))
    for name in RECALL_PTRS:
        _refused(lib, ('null pointer',), _recall(**{name: None}))


def test_nms_conditions(lib):
    _refused(lib, ('1 <= I <= 65535', 'I = 0'), _nms(I=0))
    _refused(lib, ('1 <= I <= 65535', 'I = 65536'), _nms(I=65536))
    _refused(lib, ('total', '32-bit'), _nms(total=-1, max_n=0))
    _refused(lib, ('total', '32-bit'), _nms(total=1 << 29))
    _refused(lib, ('max_n',), _nms(max_n=121))
    _refused(lib, ('max_n',), _nms(max_n=-1))
    raw = lib.raw('sn_prop_nms_workspace_bytes')
    raw.restype = ctypes.c_size_t
    need = raw(120)
    assert need >= 120 * (8 + 4 + 16)
    _refused(lib, ('short workspace', 'sn_prop_nms_workspace_bytes'), _nms(ws_bytes=need - 1))
    _refused(lib, ('short workspace',), _nms(ws=None, ws_bytes=need))
    assert raw(-1) == 0 and raw(1 << 29) == 0            # refused totals need no workspace
    assert raw(0) > 0                                     # no rows at all: still a valid pointer's worth


def test_assign_conditions(lib):
    max_gt = _limits(lib)[0]
    _refused(lib, ('I >= 1', 'I = 0'), _assign(I=0))
    _refused(lib, ('32-bit',), _assign(total=-1, max_n=0))
    _refused(lib, ('32-bit',), _assign(NG=-1))
    _refused(lib, ('32-bit',), _assign(total=1 << 29))
    _refused(lib, ('max_n',), _assign(max_n=121))
    _refused(lib, ('an image has %d ground-truth boxes' % (max_gt + 1), 'at most %d' % max_gt), _assign(max_g=max_gt + 1))
    _refused(lib, ('ground-truth boxes',), _assign(max_g=-1))


def test_recall_conditions(lib):
    max_gt, max_t = _limits(lib)[:2]
    _refused(lib, ('I >= 1', 'I = 0'), _recall(I=0))
    _refused(lib, ('1 <= A <= 8', 'A = 0'), _recall(A=0))
    _refused(lib, ('1 <= A <= 8', 'A = 9'), _recall(A=9))
    _refused(lib, ('1 <= T <= %d' % max_t, 'T = 0'), _recall(T=0))
    _refused(lib, ('1 <= T <= %d' % max_t, 'T = %d' % (max_t + 1)), _recall(T=max_t + 1))
    _refused(lib, ('32-bit',), _recall(total=-1))
    _refused(lib, ('32-bit',), _recall(NG=1 << 27, A=8))
    _refused(lib, ('an image has %d ground-truth boxes' % (max_gt + 1), 'at most %d' % max_gt), _recall(max_g=max_gt + 1))


def test_header_and_library_export_the_same_prop_symbols(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_prop_')}
    declared = {n for n in lib.protos if n.startswith('sn_prop_')}
    assert exported == declared == {'sn_prop_limits', 'sn_prop_nms_workspace_bytes', 'sn_prop_nms', 'sn_prop_assign', 'sn_prop_recall'}
