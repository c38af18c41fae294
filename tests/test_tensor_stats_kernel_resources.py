"""The compiler's resource remarks of the per-tensor statistics kernels (kept beside the object by sniper_amd/build.py): nothing in
scratch memory, nothing spilled, and the read stream runs at least four waves per SIMD in both element types."""
from sniper_amd import build as hipbuild
from test_kernel_resources import _resources


def test_tensor_stats_kernels_keep_registers_and_occupancy():
    hipbuild.build(verbose=False)
    res = _resources('tensor_stats')
    passes = {k: v for k, v in res.items() if 'tensor_stats_pass_kernel' in k}
    final = {k: v for k, v in res.items() if 'tensor_stats_finalize_kernel' in k}
    assert len(passes) == 2 and len(final) == 1, sorted(res)              # fp32 and fp16; one finalize
    for name, r in list(passes.items()) + list(final.items()):
        assert r['ScratchSize'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (name, r)
    for name, r in passes.items():
        assert r['Occupancy'] >= 4, (name, r)
