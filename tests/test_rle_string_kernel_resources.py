"""CPU: the string-count kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no
spills, no LDS -- a workgroup is one wave, DESIGN.md section 25 -- and registers few enough for full occupancy."""
from test_kernel_resources import _resources

KERNELS = ('rle_string_len_kernel', 'rle_to_string_kernel', 'rle_string_count_kernel', 'rle_from_string_kernel')


def test_rle_string_kernels_use_no_scratch_no_spills_and_no_lds():
    res = _resources('rle_string')
    assert len(res) == 4, sorted(res)
    for frag in KERNELS:
        assert any(frag in k for k in res), frag
    for name, r in res.items():
        assert any(frag in name for frag in KERNELS), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] == 0 and r['Occupancy'] == 8 and r['VGPRs'] <= 64, (name, r)
