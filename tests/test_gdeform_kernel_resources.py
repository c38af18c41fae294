"""CPU: register budgets of the grouped deformable convolution kernels (csrc/gdeform.hip), from the compiler's resource remarks."""
from test_kernel_resources import _resources


def test_gdeform_kernels_keep_everything_in_registers():
    res = _resources('gdeform')
    fwd = {k: v for k, v in res.items() if 'gdeform_fwd_kernel' in k}
    dcol = {k: v for k, v in res.items() if 'gdeform_dcol_kernel' in k}
    wgrad = {k: v for k, v in res.items() if 'gdeform_wgrad_kernel' in k}
    # forward x {fp16, fp32 offsets}; one column gradient; weight gradient x {fp16, fp32 offsets} x {Cg <= 16, Cg = 32}
    assert len(fwd) == 2 and len(dcol) == 1 and len(wgrad) == 4 and len(res) == 7, sorted(res)
    for name, r in res.items():
        # a weight fragment, corner or accumulator array indexed dynamically would move to scratch: correct results, a fraction of the speed
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
    for name, r in list(fwd.items()) + list(dcol.items()):
        # 72 registers of weight fragments + the corners of two taps in flight; sn_gdeform_fwd / _dcol put three 4-wave workgroups
        # on a CU (gd_tile_grid), i.e. three waves per SIMD: at most 168 registers
        assert r['VGPRs'] + r.get('AGPRs', 0) <= 168 and r['Occupancy'] >= 3 and r['LDS Size'] == 0, (name, r)
    for name, r in wgrad.items():
        # Cg <= 16: 72 accumulator registers, two waves per SIMD -- the two workgroups per CU the launch asks for (gc_chunk_blocks),
        # and 30 KB of LDS per workgroup allows five.  Cg = 32: 144 accumulators leave one wave per SIMD its corners in flight; the
        # launch's two workgroups per CU take turns (gdeform.hip says why), and the kernel must at least be resident
        nb2 = 'Li2E' in name
        assert r['Occupancy'] >= (1 if nb2 else 2) and r['LDS Size'] <= 32 * 1024, (name, r)
        assert r['VGPRs'] + r.get('AGPRs', 0) <= (512 if nb2 else 256), (name, r)
