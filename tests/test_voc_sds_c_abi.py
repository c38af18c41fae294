"""CPU: every argument error of the sn_vocsds_* entry points is reported before any launch, by a message that names the function and
the condition (the pointers are not dereferenced: there is no GPU here, a launch would fail with another message)."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib as load
    return load()


P = ctypes.c_void_p(16)
IOU_PTRS = ('masks', 'dt_box', 'dt_off', 'gt_bits', 'gt_pix_off', 'gt_bound', 'gt_area', 'gt_off', 'iou_off', 'dt_area', 'iou')
MATCH_PTRS = ('dt_score', 'dt_off', 'gt_off', 'iou', 'iou_off', 'iou_thrs', 'dt_best', 'dt_iou', 'dt_tp', 'dt_fp', 'gt_det')


def _iou(P_=3, M=28, thr=0.4, max_gt=20, ND=60, NG=30, n_pairs=500, max_px=1000, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_vocsds_mask_iou', g('masks'), g('dt_box'), g('dt_off'), g('gt_bits'), g('gt_pix_off'), g('gt_bound'), g('gt_area'), g('gt_off'),
            g('iou_off'), P_, M, thr, max_gt, ND, NG, n_pairs, max_px, g('dt_area'), g('iou'), None)


def _match(P_=3, T=2, max_dt=50, max_gt=20, ND=60, NG=30, **ptr):
    g = lambda k: ptr.get(k, P)
    return ('sn_vocsds_match_iou', g('dt_score'), g('dt_off'), g('gt_off'), g('iou'), g('iou_off'), g('iou_thrs'), P_, T, max_dt, max_gt, ND, NG,
            g('dt_best'), g('dt_iou'), g('dt_tp'), g('dt_fp'), g('gt_det'), None)


def _refused(lib, words, call):
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        lib.call(*call)
    msg = str(e.value)
    assert call[0] + ':' in msg and all(w in msg for w in words), msg


def test_limits_are_those_of_the_box_matching_and_admit_the_mask_head(lib):
    from sniper_amd import hip
    out = (ctypes.c_int32 * 6)()
    assert lib.call('sn_vocsds_limits', out) == 0
    max_dt, max_gt, max_t, max_m, threads, max_px = list(out)
    box = (ctypes.c_int32 * 5)()
    lib.call('sn_voc_limits', box)
    assert [max_dt, max_gt, max_t] == list(box)[:3] == [1024, 256, 8]
    assert max_m >= 28 and threads % 64 == 0 and max_px == 2 ** 31 - 1
    assert 4 * max_m * max_m + 4 * max_gt + 4 <= 64 * 1024          # the map and the counters: LDS a workgroup gets without an opt-in
    assert hip.vocsds_limits() == {'max_dt': max_dt, 'max_gt': max_gt, 'max_t': max_t, 'max_m': max_m, 'threads': threads, 'max_box_pixels': max_px}
    _refused(lib, ('null pointer',), ('sn_vocsds_limits', None))
    import re
    from sniper_amd._lib import HEADER
    with open(HEADER) as fh:
        assert re.findall(r'#define SN_VOCSDS_MAX_M (\d+)', fh.read()) == [str(max_m)]


def test_null_pointers(lib):
    for name in IOU_PTRS:
        _refused(lib, ('null pointer',), _iou(**{name: None}))
    for name in MATCH_PTRS:
        _refused(lib, ('null pointer',), _match(**{name: None}))


def test_mask_iou_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _iou(P_=0))
    _refused(lib, ('1 <= ND', 'ND = 0'), _iou(ND=0))
    _refused(lib, ('ND < 2^31',), _iou(ND=1 << 31))
    _refused(lib, ('1 <= M <= 64', 'M = 0'), _iou(M=0))
    _refused(lib, ('1 <= M <= 64', 'LDS', 'M = 65'), _iou(M=65))
    _refused(lib, ('NG < 2^31', 'NG = -1'), _iou(NG=-1))
    _refused(lib, ('a problem has 257 instances', 'at most 256'), _iou(max_gt=257))
    _refused(lib, ('a problem has -1 instances',), _iou(max_gt=-1))
    _refused(lib, ('pairs', '32-bit', 'n_pairs = 2147483648'), _iou(n_pairs=1 << 31))
    _refused(lib, ('pairs', 'n_pairs = -1'), _iou(n_pairs=-1))
    _refused(lib, ('bw * bh < 2^31', 'max_box_pixels = 2147483648'), _iou(max_px=1 << 31))
    _refused(lib, ('1 <= bw * bh', 'max_box_pixels = 0'), _iou(max_px=0))


def test_match_iou_conditions(lib):
    _refused(lib, ('P >= 1', 'P = 0'), _match(P_=0))
    _refused(lib, ('1 <= T <= 8', 'T = 0'), _match(T=0))
    _refused(lib, ('1 <= T <= 8', 'T = 9'), _match(T=9))
    _refused(lib, ('a problem has 1025 detections', 'at most 1024'), _match(max_dt=1025))
    _refused(lib, ('a problem has 257 instances', 'at most 256'), _match(max_gt=257))
    _refused(lib, ('ND >= 0',), _match(ND=-1))
    _refused(lib, ('NG >= 0',), _match(NG=-1))
    _refused(lib, ('too many rows', '32-bit'), _match(ND=1 << 28, T=8))
    _refused(lib, ('too many rows', '32-bit'), _match(NG=1 << 28, T=8))


def test_header_and_library_export_the_same_symbols(lib):
    import subprocess
    from sniper_amd._lib import LIB_PATH
    out = subprocess.run(['nm', '-D', '--defined-only', LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('sn_vocsds_')}
    declared = {n for n in lib.protos if n.startswith('sn_vocsds_')}
    assert exported == declared == {'sn_vocsds_limits', 'sn_vocsds_mask_iou', 'sn_vocsds_match_iou'}
