"""CPU: what the host-side plan answers for a ragged contraction (Cin % 64 != 0), as far as it can be asked without a launch.

Only the plain launches (sn_conv_fwd, sn_conv_dgrad) plan a ragged contraction onto the pipelined kernels, and the C ABI has no
query for those two: that the five R101 head shapes and the offset layers take the pipeline, and that Nout <= 64 does not, is read
from the kernels' phase stamps on the GPU (tests/test_gpu_conv_ragged.py), where the packed stem is checked the same way.  Rows or taps
that are not 16-byte addressable (in_ps % 8 != 0, Cin % 8 != 0) never reach the plan: the entries refuse them, which is checked here.  What IS visible here is the other half of the rule:
the queries the lowering picks its entry points by keep answering "does not qualify" for a ragged layer, so that no network's
call sequence changes (tests/test_engine_call_trace.py pins the sequences themselves), and the whole-tap answers stand."""
import pytest

# N, H, W, Cin (dx channels), Cout (the data gradient's contraction), K, pad, dil: the ragged data gradients of the R101 step
R101_RAGGED = [(20, 32, 32, 512, 72, 3, 2, 2), (20, 32, 32, 512, 48, 1, 0, 1), (20, 32, 32, 512, 88, 1, 0, 1),
               (6000, 1, 1, 1024, 88, 1, 0, 1), (6000, 1, 1, 1024, 8, 1, 0, 1), (6000, 1, 1, 12544, 104, 1, 0, 1)]


@pytest.mark.parametrize('shape', R101_RAGGED)
def test_fused_queries_do_not_qualify_a_ragged_contraction(shape):
    from sniper_amd import hip
    N, H, W, C, O, K, pad, dil = shape
    assert hip.query('sn_conv_dgrad_bn_blocks', N, H, W, C, C, O, O, 0, K, K, 1, pad, dil) == 0
    # the same layer read forward with a ragged Cin: no fused statistics, no second output, no split
    assert hip.query('sn_conv_fwd_stats_blocks', N, H, W, O, O, C, C, 0, K, K, 1, pad, dil) == 0
    assert hip.query('sn_conv_fwd_dual_ok', N, H, W, O, O, C, C, 0, K, K, 1, pad, dil, C) == 0
    assert hip.query('sn_conv_fwd_splitk_workspace_bytes', N, H, W, O, O, C, C, 0, K, K, 1, pad, dil) == 0


def test_whole_tap_answers_stand():
    from sniper_amd import hip
    assert hip.query('sn_conv_dgrad_bn_blocks', 20, 32, 32, 512, 512, 64, 64, 0, 3, 3, 1, 2, 2) == 128
    assert hip.query('sn_conv_fwd_stats_blocks', 20, 32, 32, 64, 64, 512, 512, 0, 3, 3, 1, 2, 2) == 128
    assert hip.query('sn_conv_fwd_stats_blocks', 20, 32, 32, 128, 128, 512, 512, 0, 3, 3, 1, 2, 2) == 128


@pytest.mark.parametrize('Cout,dy_ps', [(72, 76), (72, 84), (42, 42), (44, 48)])
def test_operands_that_are_not_16_byte_addressable_never_reach_a_kernel(Cout, dy_ps):
    """a data gradient whose contraction is no multiple of 8 channels (a 42-channel map at pixel stride 42) or whose rows are not
    16-byte addressable (72 channels at stride 76) is refused by the entry before any launch -- on this machine there is no GPU a
    launch could reach, and the pointers are never dereferenced -- so the ragged plan never sees it (forward alike)"""
    import ctypes
    from sniper_amd._lib import SniperHipError, lib
    p = ctypes.c_void_p(16)
    with pytest.raises(SniperHipError) as e:
        lib().call('sn_conv_dgrad', p, p, None, p, 2, 5, 7, 128, 128, Cout, dy_ps, 0, 1, 1, 1, 0, 1, 0, None)
    assert 'multiple of 8' in str(e.value)
    with pytest.raises(SniperHipError) as e:
        lib().call('sn_conv_fwd', p, p, None, None, p, 2, 5, 7, Cout, dy_ps, 128, 128, 0, 1, 1, 1, 0, 1, 0, 0, None)
    assert 'multiple of 8' in str(e.value)
