"""CPU: the PASCAL VOC evaluation kernels keep a thread's detections in registers and the problem's boxes and scores in LDS (the
compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no spills, and the 64 KB of LDS a
workgroup gets without an opt-in."""
from test_kernel_resources import _resources

KERNELS = ('voc_match_kernel', 'voc_order_kernel', 'voc_curves_kernel')


def test_voc_kernels_use_no_scratch_and_little_lds():
    res = _resources('voc_eval')
    assert len(res) == 3, sorted(res)
    for frag in KERNELS:
        assert any(frag in k for k in res), frag
    for name, r in res.items():
        assert any(frag in name for frag in KERNELS), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= 64 * 1024, (name, r)
    match = [r for k, r in res.items() if 'voc_match_kernel' in k][0]
    # half of the 64 KB (scores, order, boxes, areas, flags, the per-threshold claims): two workgroups per CU at least
    assert match['LDS Size'] <= 32 * 1024 and match['Occupancy'] >= 2, match
