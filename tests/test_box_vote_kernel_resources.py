"""CPU: the box-voting kernel keeps one kept row, its seven float64 sums and the overlap's temporaries in registers and reads the
pre-NMS rows out of LDS (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them)."""
from test_kernel_resources import _resources


def test_box_vote_kernels_use_no_scratch_and_fill_the_simd():
    """Why 8 waves per SIMD: a workgroup is ONE wave (most problems of a pass hold a few dozen rows, a wider workgroup would idle
    on them), so nothing inside a workgroup covers the latency of its LDS reads and of the float64 divide behind every overlapping
    pair -- only the waves of other workgroups on the same SIMD do.  The design plans for the most the hardware holds, 8 per SIMD
    = 32 one-wave workgroups per CU: at most 64 VGPRs, and at most 5 KB of LDS each (32 x 5 KB = the CU's 160 KB), which is where
    the chunk of 128 rows x 5 doubles comes from."""
    res = {k: v for k, v in _resources('box_vote').items() if 'box_vote_kernel' in k}
    assert len(res) == 3, sorted(res)                  # one instantiation per scoring method
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['VGPRs'] <= 64 and r['Occupancy'] == 8, (name, r)
        assert r['LDS Size'] == 128 * 5 * 8 and 32 * r['LDS Size'] <= 160 * 1024, (name, r)
