"""CPU: the mask evaluation kernels (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch,
no spills, and at most the 64 KB of LDS a workgroup gets without an opt-in."""
from test_kernel_resources import _resources

KERNELS = ('rle_stats_kernel', 'rle_iou_kernel', 'coco_match_iou_kernel')


def test_segm_kernels_use_no_scratch_and_little_lds():
    res = _resources('coco_segm')
    assert len(res) == 3, sorted(res)
    for frag in KERNELS:
        assert any(frag in k for k in res), frag
    for name, r in res.items():
        assert any(frag in name for frag in KERNELS), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= 64 * 1024, (name, r)
    match = [r for k, r in res.items() if 'coco_match_iou_kernel' in k][0]
    # scores and areas (8 B each) and order (4 B) of SN_COCO_MAX_DT = 1024 detections; 256 threads are one wave per SIMD: two
    # workgroups per CU at least, as for the box kernel
    assert match['LDS Size'] == 1024 * 20 and match['Occupancy'] >= 2, match
    for frag in ('rle_stats_kernel', 'rle_iou_kernel'):          # a wave per mask / per pair, nothing shared between waves
        assert [r for k, r in res.items() if frag in k][0]['LDS Size'] == 0


def test_polygon_and_paste_kernels_use_no_scratch_and_no_lds_to_speak_of():
    res = _resources('mask_rle')
    names = ('poly_cross_kernel', 'poly_runs_kernel', 'poly_union_kernel', 'paste_count_kernel', 'paste_fill_kernel')
    assert len(res) == 5, sorted(res)
    for name, r in res.items():
        assert any(frag in name for frag in names), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= 64, (name, r)          # one int per wave for the block sums: no sort lives in LDS
