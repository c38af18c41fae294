"""CPU: the PNG decoding and VOC ground-truth kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads
them): every kernel once, no scratch, no spills, and the LDS sn_inflate_limits reports."""
import ctypes

from test_kernel_resources import _resources


def test_png_decode_kernels_use_no_scratch_and_the_lds_the_limits_report():
    res = _resources('png_decode')
    kinds = ('inflate_kernel', 'png_unfilter_kernel', 'png_expand_kernel')
    assert len(res) == 3 and all(sum(k in name for name in res) == 1 for k in kinds), sorted(res)
    from sniper_amd._lib import lib
    lim = (ctypes.c_int32 * 6)()
    lib().call('sn_inflate_limits', lim)
    max_streams, max_bytes, lds, window, lanes, flush = list(lim)
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        if 'inflate_kernel' in name:
            # the 32 KiB window and the decoder's tables; four waves of it fit a CU's 160 KiB
            assert r['LDS Size'] == lds and window + 2048 < lds and 4 * lds <= 160 * 1024, (name, r)
        else:
            assert r['LDS Size'] == 0, (name, r)


def test_voc_gt_kernels_use_no_scratch():
    res = _resources('voc_gt')
    kinds = ('voc_inst_scan_kernel', 'voc_inst_crop_kernel')
    assert len(res) == 2 and all(sum(k in name for name in res) == 1 for k in kinds), sorted(res)
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] == (6 * 256 * 4 if 'scan' in name else 0), (name, r)          # min / max of x, y and the class per id
