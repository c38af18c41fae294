"""CPU: the proposal-roidb kernels keep a thread's columns and candidates in registers and an image's ground truth in LDS (the
compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no spills, and at most the 64 KB of LDS a
workgroup gets without an opt-in."""
from test_kernel_resources import _resources

KERNELS = ('prop_keys_kernel', 'prop_order_kernel', 'prop_nms_kernel', 'prop_assign_kernel', 'prop_recall_kernel')


def test_prop_kernels_use_no_scratch_and_little_lds():
    res = _resources('prop_roidb')
    assert len(res) == len(KERNELS), sorted(res)
    for frag in KERNELS:
        assert any(frag in k for k in res), frag
    for name, r in res.items():
        assert any(frag in name for frag in KERNELS), name
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
        assert r['LDS Size'] <= 64 * 1024, (name, r)
    recall = [r for k, r in res.items() if 'prop_recall_kernel' in k][0]
    # the compacted rows, the recorded values, the retired list and its filter: under half of the 64 KB, so two of the
    # one-workgroup-per-(image, range) problems share a CU at least
    assert recall['LDS Size'] <= 32 * 1024 and recall['Occupancy'] >= 2, recall
