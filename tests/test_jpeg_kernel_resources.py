"""CPU: the JPEG kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): the entropy decoder, the
DC scan, the IDCT and the colour kernel, no scratch, no spills, and the Huffman tables in the LDS sn_jpeg_limits reports."""
import ctypes

from test_kernel_resources import _resources


def test_jpeg_kernels_use_no_scratch_and_keep_the_tables_in_lds():
    res = _resources('jpeg_decode')
    kinds = ('jpeg_entropy_kernel', 'jpeg_dc_kernel', 'jpeg_idct_kernel', 'jpeg_colour_kernel')
    assert len(res) == 4 and all(sum(k in name for name in res) == 1 for k in kinds), sorted(res)
    from sniper_amd._lib import lib
    lim = (ctypes.c_int32 * 8)()
    lib().call('sn_jpeg_limits', lim)
    sub, threads, max_images, max_bpm, huff_lds, img_fields, seg_fields, min_sub = list(lim)
    assert threads % 64 == 0 and min_sub <= sub <= 4096 and max_images == 65535 and max_bpm == 6
    # four tables: 17 limits and 17 offsets of 4 bytes, 256 look-ahead entries of 2 bytes, 256 values
    assert huff_lds == 4 * (17 * 4 * 2 + 256 * 2 + 256)
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        if 'jpeg_entropy_kernel' in name:
            # the tables, the block scan's 256 counts, the barrier's vote
            assert huff_lds + 4 * threads <= r['LDS Size'] <= huff_lds + 4 * threads + 512, (name, r)
            assert r['Occupancy'] >= 4, (name, r)
        elif 'jpeg_idct_kernel' in name:
            assert r['LDS Size'] == 3 * 64 * 4, (name, r)          # the three quantisation tables
            assert r['Occupancy'] >= 4, (name, r)                 # 64 coefficients live in registers
        else:
            assert r['LDS Size'] == 0, (name, r)
