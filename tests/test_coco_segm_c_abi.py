"""CPU: every argument error of the sn_rle_* entry points and of sn_coco_match_iou is reported before any launch, by a message that
names the function and the condition (the pointers are not dereferenced: there is no GPU here, a launch would fail with another
message), and the library exports exactly what the header declares."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


P = ctypes.c_void_p(16)
STATS_PTRS = ('cnts', 'rle_off', 'hw', 'rows6', 'cum2')
IOU_PTRS = ('dt_cum2', 'dt_rle_off', 'dt_rows6', 'gt_cum2', 'gt_rle_off', 'gt_rows6', 'gt_flags', 'dt_off', 'gt_off', 'iou_off', 'iou')
MATCH_PTRS = ('dt', 'dt_off', 'kp_off', 'gt_area', 'gt_flags', 'gt_off', 'iou', 'iou_off', 'iou_thrs', 'area_rng', 'dt_rank', 'dt_match',
              'dt_ignore', 'gt_match', 'gt_ignore')


def _stats(N=5, total=40, max_hw=3072, score=P, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_rle_stats', g('cnts'), g('rle_off'), g('hw'), score, N, total, max_hw, g('rows6'), g('cum2'), None)


def _iou(P_=3, n_pairs=12, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_rle_iou', g('dt_cum2'), g('dt_rle_off'), g('dt_rows6'), g('gt_cum2'), g('gt_rle_off'), g('gt_rows6'), g('gt_flags'),
            g('dt_off'), g('gt_off'), g('iou_off'), P_, n_pairs, g('iou'), None)


def _match(P_=3, T=10, A=4, max_det=100, max_dt=50, max_gt=20, NK=60, NG=30, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_coco_match_iou', g('dt'), g('dt_off'), g('kp_off'), g('gt_area'), g('gt_flags'), g('gt_off'), g('iou'), g('iou_off'),
            g('iou_thrs'), g('area_rng'), P_, T, A, max_det, max_dt, max_gt, NK, NG, g('dt_rank'), g('dt_match'), g('dt_ignore'),
            g('gt_match'), g('gt_ignore'), None)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert (call[0] + ':') in msg and all(w in msg for w in words), msg


def test_limits(lib):
    out = (ctypes.c_int32 * 5)()
    assert lib.call('sn_rle_limits', out) == 0
    max_dt, max_gt, wave, per_group, threads = list(out)
    coco = (ctypes.c_int32 * 8)()
    lib.call('sn_coco_limits', coco)
    assert (max_dt, max_gt) == (coco[0], coco[1]) and max_dt >= 1024 and max_gt >= 256          # SN_COCO_MAX_DT / _GT as for boxes
    assert wave == 64 and per_group * wave == threads
    _refused(lib, ('null pointer',), ('sn_rle_limits', None))


def test_null_pointers(lib):
    for name in STATS_PTRS:
        _refused(lib, ('null pointer',), _stats(**{name: None}))
    for name in IOU_PTRS:
        _refused(lib, ('null pointer',), _iou(**{name: None}))
    for name in MATCH_PTRS:
        _refused(lib, ('null pointer',), _match(**{name: None}))


def test_stats_conditions(lib):
    _refused(lib, ('1 <= N', 'N = 0'), _stats(N=0))
    _refused(lib, ('1 <= N', 'N = 400000000'), _stats(N=400000000))
    _refused(lib, ('32-bit indexing', 'total_runs = -1'), _stats(total=-1))
    _refused(lib, ('32-bit indexing', 'total_runs = 1073741824'), _stats(total=1 << 30))
    _refused(lib, ('h * w < 2^31', 'max_hw = 2147483648'), _stats(max_hw=1 << 31))
    _refused(lib, ('h * w < 2^31', 'max_hw = 0'), _stats(max_hw=0))


def test_iou_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _iou(P_=0))
    _refused(lib, ('32-bit indexing', 'n_pairs = 2147483648'), _iou(n_pairs=1 << 31))
    _refused(lib, ('32-bit indexing', 'n_pairs = -1'), _iou(n_pairs=-1))
    assert lib.call(*_iou(n_pairs=0)) == 0                    # no pair, no launch, no error


def test_match_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _match(P_=0))
    _refused(lib, ('1 <= T <= 16', 'T = 0'), _match(T=0))
    _refused(lib, ('1 <= T <= 16', 'T = 17'), _match(T=17))
    _refused(lib, ('1 <= A <= 8', 'A = 0'), _match(A=0))
    _refused(lib, ('1 <= A <= 8', 'A = 9'), _match(A=9))
    _refused(lib, ('max_det >= 1', 'max_det = 0'), _match(max_det=0))
    _refused(lib, ('a problem has 1025 detections', 'at most 1024'), _match(max_dt=1025))
    _refused(lib, ('a problem has 257 masks of ground truth', 'at most 256'), _match(max_gt=257))
    _refused(lib, ('NK >= 0',), _match(NK=-1))
    _refused(lib, ('too many rows', '32-bit'), _match(NK=1 << 26, T=16, A=8))


def _cross(NP=3, TV=12, pts=400, max_hw=3072, fill=False, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_rle_poly_cross', g('xy'), g('poly_off'), g('edge_pt_off'), g('poly_hw'), g('cross_off') if fill else None, NP, TV, pts, max_hw,
            g('cross_count'), g('cross'), None)


def _polys(NP=3, NA=2, total=50, ws=P, ws_bytes=1 << 30, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_rle_from_polys', g('cross'), g('cross_off'), g('poly_hw'), g('ann_off'), NP, NA, total, ws, ws_bytes, g('part_runs'),
            g('part_m'), g('runs'), g('ann_m'), None)


def test_polygon_conditions(lib):
    for name in ('xy', 'poly_off', 'edge_pt_off', 'poly_hw'):
        _refused(lib, ('null pointer',), _cross(**{name: None}))
    _refused(lib, ('null pointer', 'count pass'), _cross(cross_count=None))
    _refused(lib, ('null pointer', 'fill pass'), _cross(fill=True, cross=None))
    _refused(lib, ('NP >= 1', 'NP = 0'), _cross(NP=0))
    _refused(lib, ('32-bit indexing', 'total_points = 2147483648'), _cross(pts=1 << 31))
    _refused(lib, ('32-bit indexing', 'total_vertices = 1073741824'), _cross(TV=1 << 30))
    _refused(lib, ('h * w < 2^31', 'max_hw = 2147483648'), _cross(max_hw=1 << 31))
    for name in ('cross', 'cross_off', 'poly_hw', 'ann_off', 'part_runs', 'part_m', 'runs', 'ann_m'):
        _refused(lib, ('null pointer',), _polys(**{name: None}))
    _refused(lib, ('NP >= 1 and NA >= 1', 'NA = 0'), _polys(NA=0))
    _refused(lib, ('32-bit indexing', 'total_cross = 1073741824'), _polys(total=1 << 30))
    raw = lib.raw('sn_rle_from_polys_workspace_bytes')
    need = raw(50)
    assert need >= 2 * 50 + 2 * 4 * 50 and raw(-1) == 0 and raw(1 << 30) == 0 and raw(0) > 0
    _refused(lib, ('short workspace', 'sn_rle_from_polys_workspace_bytes'), _polys(ws_bytes=need - 1))
    _refused(lib, ('short workspace',), _polys(ws=None))


def _pcount(n=4, M=28, thr=0.4, cols=100, max_hw=3072, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_rle_paste_count', g('masks'), g('boxes'), g('hw'), g('col_off'), n, M, thr, cols, max_hw, g('col_pre'), g('det_t'), None)


def _paste(n=4, M=28, thr=0.4, cols=100, runs=40, max_hw=3072, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_rle_paste', g('masks'), g('boxes'), g('hw'), g('col_off'), g('col_pre'), g('rle_off'), n, M, thr, cols, runs, max_hw,
            g('tpos'), g('cnts'), None)


def test_paste_conditions(lib):
    for name in ('masks', 'boxes', 'hw', 'col_off', 'col_pre', 'det_t'):
        _refused(lib, ('null pointer',), _pcount(**{name: None}))
    for name in ('masks', 'boxes', 'hw', 'col_off', 'col_pre', 'rle_off', 'tpos', 'cnts'):
        _refused(lib, ('null pointer',), _paste(**{name: None}))
    for call in (_pcount, _paste):
        _refused(lib, ('n >= 1', 'n = 0'), call(n=0))
        _refused(lib, ('1 <= M <= 1024', 'M = 0'), call(M=0))
        _refused(lib, ('1 <= M <= 1024', 'M = 1025'), call(M=1025))
        _refused(lib, ('n * M * M < 2^31',), call(n=4096, M=1024))
        _refused(lib, ('32-bit indexing', 'total_cols = 2147483648'), call(cols=1 << 31))
        _refused(lib, ('h * w < 2^31', 'max_hw = 2147483648'), call(max_hw=1 << 31))
    _refused(lib, ('n <= total_runs < 2^30', 'total_runs = 3'), _paste(runs=3))
    _refused(lib, ('n <= total_runs < 2^30', 'total_runs = 1073741824'), _paste(runs=1 << 30))


def test_header_and_library_export_the_same_symbols(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_')}
    assert exported == set(lib.protos), (sorted(exported - set(lib.protos)), sorted(set(lib.protos) - exported))
    assert {'sn_rle_limits', 'sn_rle_stats', 'sn_rle_iou', 'sn_coco_match_iou', 'sn_rle_poly_cross', 'sn_rle_from_polys',
            'sn_rle_from_polys_workspace_bytes', 'sn_rle_paste_count', 'sn_rle_paste'} <= exported
