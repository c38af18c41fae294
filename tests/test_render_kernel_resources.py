"""CPU: the render kernel (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): exactly the two forms of
the one kernel, no scratch, no spills, and an LDS list of the size sn_render_limits reports."""
import ctypes

from test_kernel_resources import _resources


def test_render_kernels_use_no_scratch_and_the_lds_list_only():
    res = _resources('render')
    assert len(res) == 2 and all('render_kernel' in k for k in res), sorted(res)          # the uint8 form and the tensor form
    assert len({k for k in res if 'ILb0E' in k}) == 1 and len({k for k in res if 'ILb1E' in k}) == 1, sorted(res)
    from sniper_amd._lib import lib
    lim = (ctypes.c_int32 * 5)()
    lib().call('sn_render_limits', lim)
    per_round, threads = lim[3], lim[4]
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= 64 * 1024, (name, r)
        # the list (a 32-byte entry per slot: rect, colour, mask row, text range), one survivor count per wave, the seven table addresses
        assert r['LDS Size'] == 32 * per_round + 4 * (threads // 64) + 8 * 7, (name, r)
        # a memory-bound pass wants waves in flight: at least 4 per SIMD
        assert r['Occupancy'] >= 4, (name, r)
