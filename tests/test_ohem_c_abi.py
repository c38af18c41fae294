"""CPU: sn_box_annotator_ohem is exported, and every argument it refuses is refused by name before any launch (NULL stream, no
device: the pointers are never dereferenced)."""
import ctypes

import pytest

from test_c_abi import lib  # noqa: F401  (the module-scoped fixture that builds and loads the library)

MAX_ROIS = 16384        # SN_OHEM_MAX_ROIS of include/sniper_hip.h: one image's keys in the 64 KB of LDS a workgroup gets


def _call(lib, B=2, R=300, C=81, box_dim=4, k=128, ptr=ctypes.c_void_p(16), null=None):  # noqa: F811
    args = [ptr] * 7 + [None]
    if null is not None:
        args[null] = None
    return lib.call('sn_box_annotator_ohem', *args, B, R, C, box_dim, k, None)


def test_entry_point_is_exported_with_its_prototype(lib):  # noqa: F811
    ret, argtypes, names = lib.protos['sn_box_annotator_ohem']
    assert names == ['cls_score', 'bbox_pred', 'labels', 'bbox_targets', 'bbox_weights', 'labels_ohem', 'bbox_weights_ohem',
                     'fg_labels', 'B', 'R', 'C', 'box_dim', 'roi_per_img', 'stream']
    assert ret is ctypes.c_int and argtypes == [ctypes.c_void_p] * 8 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert hasattr(lib.raw('sn_box_annotator_ohem'), 'argtypes')
    hdr = open(__import__('sniper_amd._lib', fromlist=['HEADER']).HEADER).read()
    assert '#define SN_OHEM_MAX_ROIS %d' % MAX_ROIS in hdr and MAX_ROIS >= 6000          # RPN_PRE_NMS_TOP_N fits


@pytest.mark.parametrize('kw,words', [
    (dict(k=0), ('roi_per_img >= 1', 'roi_per_img = 0')),
    (dict(k=-3), ('roi_per_img >= 1', 'roi_per_img = -3')),
    (dict(C=1), ('C >= 2', 'C = 1')),
    (dict(box_dim=0), ('box_dim >= 1', 'box_dim = 0')),
    (dict(B=0), ('B >= 1', 'B = 0')),
    (dict(R=0), ('R >= 1', 'R = 0')),
    (dict(R=MAX_ROIS + 1), ('R <= %d' % MAX_ROIS, 'LDS', 'R = %d' % (MAX_ROIS + 1))),
    (dict(null=0), ('null pointer',)),
    (dict(null=6), ('null pointer',)),
])
def test_refused_arguments(lib, kw, words):  # noqa: F811
    from sniper_amd._lib import SniperHipError
    with pytest.raises(SniperHipError) as e:
        _call(lib, **kw)
    msg = str(e.value)
    assert 'sn_box_annotator_ohem' in msg and all(w in msg for w in words), msg
