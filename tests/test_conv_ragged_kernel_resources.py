"""CPU: the RAGGED instantiations of the pipelined convolution (csrc/conv_dma_ragged.hip) keep their accumulators in registers
(the compiler's own resource remarks, as tests/test_kernel_resources.py reads them): no scratch, no spilled vector registers, and
the waves per SIMD of the whole-tap configurations they stand in for."""
from test_kernel_resources import _resources


def test_ragged_kernels_use_no_scratch():
    res = {k: v for k, v in _resources('conv_dma_ragged').items() if 'conv_dma_ragged_kernel' in k}
    # data gradient: 64 x 128 two-stage (6) and 160 x 128 with 8 waves (16); forward: 6 and 160 x 128 with 4 waves (14)
    assert len(res) == 4, sorted(res)
    whole = {k: v for k, v in _resources('conv_dma').items() if 'conv_dma_kernel' in k}
    for name, r in res.items():
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0, (name, r)
        twin = whole[name.replace('conv_dma_ragged_kernel', 'conv_dma_kernel').replace('_Z22', '_Z15')]
        assert r['Occupancy'] == twin['Occupancy'] and r['LDS Size'] == twin['LDS Size'], (name, r, twin)
