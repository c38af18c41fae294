"""CPU: the COCO evaluation kernels keep a lane's boxes and matched state in registers and rank out of LDS (the compiler's own
resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no spills, and the 64 KB of LDS a workgroup gets without
an opt-in."""
from test_kernel_resources import _resources

KERNELS = ('coco_match_kernel', 'coco_pack_rows_kernel', 'coco_keys_kernel', 'coco_order_kernel', 'coco_curves_kernel')


def test_coco_kernels_use_no_scratch_and_little_lds():
    res = _resources('coco_eval')
    assert len(res) == 6, sorted(res)                  # the five kernels, the row packing for float32 and for float64
    for frag in KERNELS:
        assert any(frag in k for k in res), frag
    for name, r in res.items():
        assert any(frag in name for frag in KERNELS), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= 64 * 1024, (name, r)
    match = [r for k, r in res.items() if 'coco_match_kernel' in k][0]
    # scores (8 B) and order (4 B) of SN_COCO_MAX_DT = 1024 detections; 256 threads are one wave per SIMD: two workgroups per CU at least
    assert match['LDS Size'] == 1024 * 12 and match['Occupancy'] >= 2, match
