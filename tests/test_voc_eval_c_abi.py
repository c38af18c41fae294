"""CPU: every argument error of the sn_voc_* entry points is reported before any launch, by a message that names the function and the
condition (the pointers are not dereferenced: there is no GPU here, a launch would fail with another message)."""
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
WS = 1 << 30
MATCH_PTRS = ('dt_box', 'dt_score', 'dt_off', 'gt_box', 'gt_difficult', 'gt_off', 'iou_thrs', 'dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det')
ACC_PTRS = ('dt_score', 'dt_off', 'gt_off', 'cat_off', 'gt_difficult', 'dt_tp', 'dt_fp', 'h_ap07_thrs', 'order', 'rec', 'prec', 'npos', 'ap07',
            'ap_area')
THRS = np.arange(0., 1.1, 0.1)


def _match(P_=3, T=2, max_dt=50, max_gt=20, ND=60, NG=30, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_voc_match', g('dt_box'), g('dt_score'), g('dt_off'), g('gt_box'), g('gt_difficult'), g('gt_off'), g('iou_thrs'), P_, T, max_dt,
            max_gt, ND, NG, g('dt_best'), g('dt_iou'), g('dt_tp'), g('dt_fp'), g('gt_det'), None)


def _acc(P_=3, K=5, T=2, max_cls=40, ND=60, NG=30, ws=P, ws_bytes=WS, **ptr):
    g = lambda k: ptr.get(k, P)
    h_thr = ptr['h_ap07_thrs'] if 'h_ap07_thrs' in ptr else ctypes.c_void_p(THRS.ctypes.data)
    return ('sn_voc_accumulate', g('dt_score'), g('dt_off'), g('gt_off'), g('cat_off'), g('gt_difficult'), g('dt_tp'), g('dt_fp'), h_thr, P_, K, T,
            max_cls, ND, NG, ws, ws_bytes, g('order'), g('rec'), g('prec'), g('npos'), g('ap07'), g('ap_area'), None)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert call[0] + ':' in msg and all(w in msg for w in words), msg


def test_limits_admit_what_the_issue_asks(lib):
    out = (ctypes.c_int32 * 5)()
    assert lib.call('sn_voc_limits', out) == 0
    max_dt, max_gt, max_t, tile, chunk = list(out)
    assert max_dt >= 1024 and max_gt >= 256 and max_t >= 8 and tile >= 64 and chunk >= 64
    _refused(lib, ('null pointer',), ('sn_voc_limits', None))
    import re
    from sniper_amd._lib import HEADER
    with open(HEADER) as fh:
        defs = dict(re.findall(r'#define (SN_VOC_MAX_\w+) (\d+)', fh.read()))
    assert defs == {'SN_VOC_MAX_DT': str(max_dt), 'SN_VOC_MAX_GT': str(max_gt), 'SN_VOC_MAX_T': str(max_t)}


def test_null_pointers(lib):
    for name in MATCH_PTRS:
        _refused(lib, ('null pointer',), _match(**{name: None}))
    for name in ACC_PTRS:
        _refused(lib, ('null pointer',), _acc(**{name: None}))


def test_match_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _match(P_=0))
    _refused(lib, ('1 <= T <= 8', 'T = 0'), _match(T=0))
    _refused(lib, ('1 <= T <= 8', 'T = 9'), _match(T=9))
    _refused(lib, ('a problem has 1025 detections', 'at most 1024'), _match(max_dt=1025))
    _refused(lib, ('a problem has 257 boxes', 'at most 256'), _match(max_gt=257))
    _refused(lib, ('ND >= 0',), _match(ND=-1))
    _refused(lib, ('NG >= 0',), _match(NG=-1))
    _refused(lib, ('too many rows', '32-bit'), _match(ND=1 << 28, T=8))
    _refused(lib, ('too many rows', '32-bit'), _match(NG=1 << 28, T=8))


def test_accumulate_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _acc(P_=0))
    _refused(lib, ('1 <= K', 'K = 0'), _acc(K=0))
    _refused(lib, ('K <= 65535', 'K = 65536'), _acc(K=65536))
    _refused(lib, ('1 <= T <= 8', 'T = 0'), _acc(T=0))
    _refused(lib, ('1 <= T <= 8', 'T = 9'), _acc(T=9))
    _refused(lib, ('ND >= 0',), _acc(ND=-1, max_cls=0))
    _refused(lib, ('max_dt_per_class',), _acc(max_cls=61))
    _refused(lib, ('max_dt_per_class',), _acc(max_cls=-1))
    _refused(lib, ('too many rows', '32-bit'), _acc(ND=1 << 28, T=8))


def test_short_workspace(lib):
    raw = lib.raw('sn_voc_accumulate_workspace_bytes')
    need = raw(60, 2)
    assert need >= 2 * 60 * 8
    _refused(lib, ('short workspace', 'sn_voc_accumulate_workspace_bytes'), _acc(ws_bytes=need - 1))
    _refused(lib, ('short workspace',), _acc(ws=None, ws_bytes=need))
    assert raw(60, 9) == 0 and raw(60, 0) == 0 and raw(-1, 2) == 0          # refused shapes need no workspace
    assert raw(0, 1) > 0                                                   # no detections at all: still a valid pointer's worth


def test_header_and_library_export_the_same_voc_symbols(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_voc_')}
    declared = {n for n in lib.protos if n.startswith('sn_voc_')}
    assert exported == declared == {'sn_voc_limits', 'sn_voc_match', 'sn_voc_accumulate', 'sn_voc_accumulate_workspace_bytes'}
