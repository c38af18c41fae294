"""CPU: every argument error of the sn_coco_* entry points is reported before any launch, by a message that names the condition (the
pointers are not dereferenced: there is no GPU here, a launch would fail with another message)."""
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
MATCH_PTRS = ('dt', 'dt_off', 'kp_off', 'gt', 'gt_flags', 'gt_off', 'iou_thrs', 'area_rng', 'dt_rank', 'dt_match', 'dt_ignore', 'gt_match',
              'gt_ignore')
ACC_PTRS = ('dt', 'dt_off', 'kp_off', 'gt_off', 'cat_off', 'dt_rank', 'dt_match', 'dt_ignore', 'gt_ignore', 'rec_thrs', 'precision',
            'recall')


def _match(P_=3, T=10, A=4, max_det=100, max_dt=50, max_gt=20, NK=60, NG=30, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_coco_match', g('dt'), g('dt_off'), g('kp_off'), g('gt'), g('gt_flags'), g('gt_off'), g('iou_thrs'), g('area_rng'), P_, T, A,
            max_det, max_dt, max_gt, NK, NG, g('dt_rank'), g('dt_match'), g('dt_ignore'), g('gt_match'), g('gt_ignore'), None)


def _acc(P_=3, K=5, T=10, A=4, R=101, max_det=100, max_dets=(1, 10, 100), M=None, max_cat=40, NK=60, NG=30, ws=P, ws_bytes=WS, **ptr):
    g = lambda k: ptr.get(k, P)
    md = np.asarray(max_dets, np.int32)
    h_md = ptr['h_max_dets'] if 'h_max_dets' in ptr else ctypes.c_void_p(md.ctypes.data)
    call = ('sn_coco_accumulate', g('dt'), g('dt_off'), g('kp_off'), g('gt_off'), g('cat_off'), g('dt_rank'), g('dt_match'), g('dt_ignore'),
            g('gt_ignore'), g('rec_thrs'), h_md, P_, K, T, A, len(md) if M is None else M, R, max_det, max_cat, NK, NG, ws, ws_bytes,
            g('precision'), g('recall'), None)
    return call, md          # md: kept alive by the caller until the call has read it


def _refused(lib, words, call, keep=None):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert call[0] in msg and all(w in msg for w in words), msg


def test_limits_admit_what_the_issue_asks(lib):
    out = (ctypes.c_int32 * 8)()
    assert lib.call('sn_coco_limits', out) == 0
    max_dt, max_gt, max_t, max_a, max_m, max_r, tile, chunk = list(out)
    assert max_dt >= 1024 and max_gt >= 256 and max_t >= 16 and max_a >= 8 and max_m >= 4 and max_r >= 128
    assert tile >= 64 and chunk >= 64
    _refused(lib, ('null pointer',), ('sn_coco_limits', None))


def test_null_pointers(lib):
    for name in MATCH_PTRS:
        _refused(lib, ('null pointer',), _match(**{name: None}))
    for name in ACC_PTRS + ('h_max_dets',):
        call, md = _acc(**{name: None})
        _refused(lib, ('null pointer',), call)
    _refused(lib, ('null pointer',), ('sn_coco_pack_rows', None, 0, None, 4, P, None))
    _refused(lib, ('null pointer',), ('sn_coco_pack_rows', P, 0, None, 4, None, None))


def test_match_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _match(P_=0))
    _refused(lib, ('1 <= T <= 16', 'T = 0'), _match(T=0))
    _refused(lib, ('1 <= T <= 16', 'T = 17'), _match(T=17))
    _refused(lib, ('1 <= A <= 8', 'A = 0'), _match(A=0))
    _refused(lib, ('1 <= A <= 8', 'A = 9'), _match(A=9))
    _refused(lib, ('max_det >= 1', 'max_det = 0'), _match(max_det=0))
    _refused(lib, ('a problem has 1025 detections', 'at most 1024'), _match(max_dt=1025))
    _refused(lib, ('a problem has 257 boxes', 'at most 256'), _match(max_gt=257))
    _refused(lib, ('NK >= 0',), _match(NK=-1))
    _refused(lib, ('too many rows', '32-bit'), _match(NK=1 << 26, T=16, A=8))


def test_accumulate_conditions(lib):
    def no(words, **kw):
        call, md = _acc(**kw)
        _refused(lib, words, call)
    no(('P >= 1', 'P = 0'), P_=0)
    no(('1 <= K', 'K = 0'), K=0)
    no(('1 <= T <= 16', 'T = 17'), T=17)
    no(('1 <= T <= 16', 'T = 0'), T=0)
    no(('1 <= A <= 8', 'A = 9'), A=9)
    no(('1 <= A <= 8', 'A = 0'), A=0)
    no(('1 <= M <= 4', 'M = 0'), M=0)
    no(('1 <= M <= 4', 'M = 5'), max_dets=(1, 2, 3, 4, 100))
    no(('1 <= R <= 128', 'R = 0'), R=0)
    no(('1 <= R <= 128', 'R = 129'), R=129)
    no(('max_det >= 1', 'max_det = 0'), max_det=0)
    no(('max_dets[0] >= 1',), max_dets=(0, 10, 100))
    no(('max_dets must be ascending', 'max_dets[2] = 10 after 10'), max_dets=(1, 10, 10), max_det=10)
    no(('max_dets must be ascending',), max_dets=(10, 1, 100))
    no(('the last of max_dets must equal max_det', '50 != 100'), max_dets=(1, 10, 50))
    no(('max_kept_per_category',), max_cat=61)
    no(('too many rows', '32-bit'), NK=1 << 26, T=16, A=8, max_cat=0)


def test_short_workspace(lib):
    raw = lib.raw('sn_coco_accumulate_workspace_bytes')
    need = raw(60, 10, 4)
    assert need >= 60 * (8 + 4 + 4) + 40 * 60 * (4 + 8)
    call, md = _acc(ws_bytes=need - 1)
    _refused(lib, ('short workspace', 'sn_coco_accumulate_workspace_bytes'), call)
    call, md = _acc(ws=None, ws_bytes=need)
    _refused(lib, ('short workspace',), call)
    assert raw(60, 17, 4) == 0 and raw(60, 10, 9) == 0 and raw(-1, 10, 4) == 0          # refused shapes need no workspace
    assert lib.raw('sn_coco_match_workspace_bytes')() == 0


def test_pack_rows_conditions(lib):
    _refused(lib, ('1 <= n', 'n = 0'), ('sn_coco_pack_rows', P, 0, None, 0, P, None))
    _refused(lib, ('rows_f32 must be 0', 'got 2'), ('sn_coco_pack_rows', P, 2, None, 4, P, None))


def test_header_and_library_export_the_same_coco_symbols(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_')}
    assert exported == set(lib.protos), (sorted(exported - set(lib.protos)), sorted(set(lib.protos) - exported))
    assert {'sn_coco_limits', 'sn_coco_match', 'sn_coco_match_workspace_bytes', 'sn_coco_accumulate', 'sn_coco_accumulate_workspace_bytes',
            'sn_coco_pack_rows'} <= exported
