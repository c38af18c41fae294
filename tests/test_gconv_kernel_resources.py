"""CPU: register budgets of the grouped-convolution kernels (csrc/gconv.hip and the ordered partial sum its weight gradient
finishes with, csrc/common.hip), from the compiler's resource remarks."""
from test_kernel_resources import _resources


def test_gconv_kernels_keep_everything_in_registers():
    res = _resources('gconv')
    res.update({k: v for k, v in _resources('common').items() if 'partial_sum_kernel' in k})
    mfma = {k: v for k, v in res.items() if 'gconv_mfma_kernel' in k}
    wgrad = {k: v for k, v in res.items() if 'gconv_wgrad_mfma_kernel' in k}
    plain = {k: v for k, v in res.items() if 'gconv_plain_' in k or 'partial_sum_kernel' in k}
    assert len(mfma) == 4 and len(wgrad) == 4 and len(plain) == 4, sorted(res)       # {1x1, 3x3} x {fwd, dgrad}; {1x1, 3x3} x {Cg<=16, 32}
    assert len(res) == 12, sorted(res)
    for name, r in res.items():
        # a weight fragment or accumulator array indexed dynamically would move to scratch: correct results at a fraction of the speed
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
    for name, r in mfma.items():
        # 3x3: 72 registers of weight fragments + 36 of activation fragments + 8 accumulators + addresses.  The forward launch puts
        # three 4-wave workgroups on a CU (gc_launch_mfma), i.e. three waves per SIMD: at most 168 registers
        assert r['VGPRs'] <= 168 and r['Occupancy'] >= 3, (name, r)
    for name, r in wgrad.items():
        # 3x3 with Cg = 32: 9 taps x 4 blocks x 4 = 144 accumulator registers beside the fragments; the launch asks for two
        # workgroups per CU (gc_wgrad_blocks), i.e. two waves per SIMD, and 30 KB of LDS per workgroup allows five
        assert r['Occupancy'] >= 2 and r['LDS Size'] <= 32 * 1024, (name, r)
