"""CPU: the BoxAnnotatorOHEM kernel keeps a row's scores, its box terms and the prefetched next row in registers and ranks out of
LDS (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no spills."""
from test_kernel_resources import _resources


def test_ohem_kernel_uses_no_scratch():
    res = {k: v for k, v in _resources('ohem').items() if 'box_annotator_ohem_kernel' in k}
    assert len(res) == 1, sorted(res)                  # "at most two launches": it is one kernel
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        # a 1024-thread workgroup is 4 waves per SIMD: at most 128 registers each
        assert r['VGPRs'] <= 128 and r['Occupancy'] >= 4, (name, r)
