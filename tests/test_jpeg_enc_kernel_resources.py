"""CPU: the JPEG encoder's kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): the blocks, size,
write and the two stuffing kernels use no scratch and have no spills -- the 64 values of a block stay in registers -- and their LDS
is what sn_jpeg_enc_limits reports."""
import ctypes

from test_kernel_resources import _resources


def test_jpeg_enc_kernels_use_no_scratch_and_the_lds_the_limits_report():
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    res = _resources('jpeg_encode')
    kinds = ('jpeg_enc_blocks_kernel', 'jpeg_enc_size_kernel', 'jpeg_enc_write_kernel', 'jpeg_enc_stuff_kernelILi1E', 'jpeg_enc_stuff_kernelILi2E')
    assert len(res) == 5 and all(sum(k in name for name in res) == 1 for k in kinds), sorted(res)
    from sniper_amd._lib import lib
    lim = (ctypes.c_int32 * 8)()
    lib().call('sn_jpeg_enc_limits', lim)
    threads, max_pictures, max_blocks, raw_per_block, chunk, blocks_lds, code_lds, stuffed_per_raw = list(lim)
    assert threads % 64 == 0 and max_pictures == 65535 and max_blocks == 1 << 22 and chunk == 64 and stuffed_per_raw == 2
    assert raw_per_block == (22 + 63 * 26 + 7) // 8 == 208
    assert blocks_lds == 2 * 2 * 64 * 4               # a divisor and its reciprocal per entry of two tables
    assert code_lds == (2 * 16 + 2 * 256) * 4         # a code and its length per symbol of two DC and two AC tables
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        if 'blocks_kernel' in name:
            assert r['LDS Size'] == blocks_lds and r['VGPRs'] >= 64 and r['Occupancy'] >= 2, (name, r)
        elif 'size_kernel' in name or 'write_kernel' in name:
            assert r['LDS Size'] == code_lds and r['Occupancy'] >= 4, (name, r)
        else:
            assert r['LDS Size'] == 0, (name, r)
