"""CPU: the PNG kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): the filter, the plan and
the two deflate kernels, no scratch, no spills, and the LDS sn_deflate_limits reports."""
import ctypes

from test_kernel_resources import _resources


def test_png_kernels_use_no_scratch_and_the_lds_the_limits_report():
    res = _resources('png_encode')
    kinds = ('png_filter_kernel', 'deflate_plan_kernel', 'deflate_code_kernel', 'deflate_write_kernel')
    assert len(res) == 4 and all(sum(k in name for name in res) == 1 for k in kinds), sorted(res)
    from sniper_amd._lib import lib
    lim = (ctypes.c_int32 * 6)()
    lib().call('sn_deflate_limits', lim)
    block, threads, max_streams, code_words, code_lds, write_lds = list(lim)
    assert 8192 <= block <= 65535 and threads % 64 == 0 and block == 64 * threads          # a 64-bit word of run flags per thread
    assert max_streams == 65535 and code_words >= 286 + 72 + 5
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        if 'deflate_code_kernel' in name:
            # the block's bytes, a flag bit per byte, and the code construction's tables
            assert r['LDS Size'] == code_lds and block + block // 8 < code_lds <= 64 * 1024, (name, r)
            assert r['Occupancy'] >= 4, (name, r)
        else:
            assert r['LDS Size'] == 0, (name, r)           # (the write kernel's LDS is dynamic: sized at the launch)
    # the write kernel: the block's bytes, its coded image, the flags, the code -- above the 64 KiB default, inside the CU's 160 KiB
    assert 2 * block + block // 8 + 4 * 286 < write_lds <= 160 * 1024
