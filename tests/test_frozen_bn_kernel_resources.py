"""CPU: the frozen-BatchNorm backward kernels keep their per-channel coefficients, partial sums and the four row loads in flight
in registers (the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no spills."""
from test_kernel_resources import _resources


def test_frozen_bn_kernels_use_no_scratch():
    nn = _resources('nn_ops')
    bwd = {k: v for k, v in nn.items() if 'bn_frozen_bwd_kernel' in k}
    assert len(bwd) == 3, sorted(bwd)              # dx + parameter gradients, parameter gradients only, dx only
    others = {k: v for k, v in nn.items() if 'bn_frozen_finalize_kernel' in k or 'bn_global_batch_kernel' in k}
    assert len(others) == 2, sorted(others)
    for name, res in list(bwd.items()) + list(others.items()):
        assert res['ScratchSize'] == 0 and res['VGPRs Spill'] == 0 and res['SGPRs Spill'] == 0, (name, res)
    # at least three 256-thread workgroups per CU (<= 168 registers): with 12 16-byte loads per thread in flight that is ~147 KB
    # outstanding per CU, well beyond what the HBM latency-bandwidth product asks of one CU
    for name, res in bwd.items():
        assert res['VGPRs'] <= 168 and res['Occupancy'] >= 3, (name, res)
