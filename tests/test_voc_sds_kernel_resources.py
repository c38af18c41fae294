"""CPU: the PASCAL VOC mask evaluation kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no
scratch, no spills, and the LDS that DESIGN.md section 24 states."""
from test_kernel_resources import _resources

KERNELS = ('voc_mask_iou_kernel', 'voc_match_iou_kernel')


def test_voc_sds_kernels_use_no_scratch_and_the_lds_the_design_states():
    res = _resources('voc_segm')
    assert len(res) == 2, sorted(res)
    for frag in KERNELS:
        assert any(frag in k for k in res), frag
    for name, r in res.items():
        assert any(frag in name for frag in KERNELS), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
    iou = [r for k, r in res.items() if 'voc_mask_iou_kernel' in k][0]
    # the 64 x 64 float32 map (SN_VOCSDS_MAX_M), one counter per instance of the problem (SN_VOC_MAX_GT) and the area: three
    # workgroups per CU by LDS alone would already fill it with waves (256 threads = one wave per SIMD)
    assert iou['LDS Size'] == 4 * 64 * 64 + 4 * 256 + 4 and iou['Occupancy'] >= 4, iou
    match = [r for k, r in res.items() if 'voc_match_iou_kernel' in k][0]
    # scores (8 B) and order (4 B) of SN_VOC_MAX_DT = 1024 detections, the thresholds, the per-threshold claims of 256 instances
    assert match['LDS Size'] == 1024 * 12 + 8 * 8 + 4 * 8 * 256 and match['Occupancy'] >= 2, match
