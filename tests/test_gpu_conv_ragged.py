"""-m gpu: convolutions whose contraction per tap is a multiple of 8 channels but not of 64 on the LDS-DMA pipelined kernels
(conv_dma_ragged_kernel, csrc/conv_dma_ragged.hip): a tap's last K-step is partial and the lanes beyond Cin must read zeros for
both operands.  sn_conv_dgrad (whose contraction is the layer's output width: the 72-channel offset layers, the RPN / R-CNN heads)
and sn_conv_fwd against torch-CPU fp32 on the same fp16-rounded operands, at the tolerance of test_gpu_nn_ops.py's data-gradient
tests; which kernel ran is read from the pipelined kernel's phase stamps (sn_conv_trace: conv_igemm_kernel writes none)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

pytestmark = pytest.mark.gpu

from gpu_util import Stamps as _Stamps, assert_close, dev, f16r, from_nhwc, to_nhwc_f16, w_to_otI  # noqa: E402

# name -> N, H, W (of dx), dx channels, contraction (= dy channels), K, stride, pad, dilation
CASES = {
    'm64': (1, 8, 8, 128, 72, 3, 1, 2, 2),          # M = 64: less than one row tile of any configuration
    'rows': (2, 5, 7, 128, 72, 3, 1, 2, 2),         # M = 70: ragged rows; two K-steps per tap, the second 8 of 64
    'k8': (2, 5, 7, 128, 8, 1, 1, 0, 1),            # one K-step, 56 of its 64 channels zero-filled
    'k136': (2, 5, 7, 128, 136, 1, 1, 0, 1),        # two whole steps and a ragged one
    'k200': (2, 5, 7, 128, 200, 3, 1, 1, 1),        # last step 8 of 64, nine taps
    'tiles': (3, 9, 11, 136, 72, 3, 1, 2, 2),       # several row tiles, two column tiles (the second 8 of 128 channels)
    's2': (2, 10, 14, 128, 72, 3, 2, 1, 1),         # stride 2: the walk by parity class with ragged taps
    'control64': (2, 5, 7, 128, 64, 3, 1, 1, 1),    # whole taps: the unchanged path
}


def _hip():
    from sniper_amd import hip
    return hip


@pytest.fixture
def conv_tuning():
    hip = _hip()
    yield hip
    hip.call('sn_conv_tune', -1)
    hip.call('sn_conv_trace', None)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """operands and the fp32 reference of a case, computed once: (dy (N,O,Ho,Wo), w (O,C,K,K), want dx (N,C,H,W))"""
    N, H, W, C, O, K, s, p, d = CASES[name]
    rs = np.random.RandomState(sorted(CASES).index(name) + 11)
    w = f16r(rs.standard_normal((O, C, K, K)) / np.sqrt(O * K * K))
    xt = torch.zeros((N, C, H, W), requires_grad=True)
    y = Fnn.conv2d(xt, torch.from_numpy(w), None, s, p, d)
    dy = f16r(rs.standard_normal(tuple(y.shape)))
    y.backward(torch.from_numpy(dy))
    want = xt.grad.numpy().copy()
    for a in (w, dy, want):
        a.setflags(write=False)
    return dy, w, want


def _dgrad(name, dy_ps=None, spare=0.0):
    """sn_conv_dgrad of a case; dy rows of `dy_ps` halves (default: the contraction itself), the spare halves filled with `spare`"""
    hip = _hip()
    N, H, W, C, O, K, s, p, d = CASES[name]
    dy, w, _ = _problem(name)
    Ho, Wo = dy.shape[2], dy.shape[3]
    ps = dy_ps or O
    d_dy = torch.full((N, Ho, Wo, ps), spare, dtype=torch.float16, device=dev())
    d_dy[..., :O] = to_nhwc_f16(dy)
    w_otI = torch.from_numpy(w_to_otI(w)).to(dev())
    wT = torch.empty((C, K * K, O), dtype=torch.float16, device=dev())
    hip.call('sn_weight_transpose', w_otI, wT, O, K * K, C, O, hip.stream())
    dx = torch.full((N, H, W, C), 777.0, dtype=torch.float16, device=dev())
    hip.call('sn_conv_dgrad', d_dy, wT, None, dx, N, H, W, C, C, O, ps, C, K, K, s, p, d, 0, hip.stream())
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize('cfg', [-1, 6, 16])
@pytest.mark.parametrize('name', sorted(CASES))
def test_ragged_dgrad_against_cpu(name, cfg, conv_tuning):
    """the built-in choice and both RAGGED data-gradient configurations forced (sn_conv_tune), against the fp32 reference"""
    conv_tuning.call('sn_conv_tune', cfg)
    want = _problem(name)[2]
    dx = _dgrad(name)          # the launch as the engine makes it: no trace buffer installed
    assert_close(from_nhwc(dx), want, 1e-2, 1e-2 * np.abs(want).max(), 'ragged dgrad %s cfg %d' % (name, cfg))
    st = _Stamps()
    with st:
        traced = _dgrad(name)      # (with stamps the kernel also drains its stores before the statistics phase)
    assert st.pipelined, 'case %s cfg %d ran conv_igemm_kernel' % (name, cfg)
    assert torch.equal(dx.view(torch.int16), traced.view(torch.int16))


@pytest.mark.parametrize('name', ['rows', 'tiles', 'k200'])
def test_ragged_dgrad_equals_register_staged_kernel(name, conv_tuning):
    """cross-path: the pipelined result and conv_igemm_kernel's (sn_conv_tune(0)) on the same inputs"""
    want = _problem(name)[2]
    st = _Stamps()
    with st:
        pipe = from_nhwc(_dgrad(name))
    assert st.pipelined
    conv_tuning.call('sn_conv_tune', 0)
    with st:
        staged = from_nhwc(_dgrad(name))
    assert not st.pipelined, 'sn_conv_tune(0) did not select conv_igemm_kernel'
    top = np.abs(want).max()
    assert_close(staged, want, 1e-2, 1e-2 * top, 'register-staged dgrad %s' % name)
    assert_close(pipe, staged, 1e-2, 1e-2 * top, 'pipelined vs register-staged dgrad %s' % name)


@pytest.mark.parametrize('cfg', [-1, 6, 16])
@pytest.mark.parametrize('spare', [60000.0, float('nan')])
def test_ragged_dgrad_ignores_the_row_padding(spare, cfg, conv_tuning):
    """dy rows of 80 halves for a 72-channel contraction, the 8 spare halves large or NaN: the chunk beyond Cin must be zero-filled
    (a NaN that reaches an MFMA poisons the output whatever the other operand holds), so dx is bit-equal to the packed run"""
    conv_tuning.call('sn_conv_tune', cfg)
    for name in ('rows', 'tiles'):
        packed = _dgrad(name)
        padded = _dgrad(name, dy_ps=80, spare=spare)
        assert torch.equal(packed.view(torch.int16), padded.view(torch.int16)), (name, cfg, spare)
        want = _problem(name)[2]
        assert_close(from_nhwc(padded), want, 1e-2, 1e-2 * np.abs(want).max(), 'ragged dgrad, padded rows %s cfg %d' % (name, cfg))


@pytest.mark.parametrize('cfg', [-1, 6, 14])
def test_ragged_forward(cfg, conv_tuning):
    """sn_conv_fwd, Cin = 72, 3 x 3, 2 x 5 x 7 pixels, with bias + ReLU: packed rows, and rows of 80 halves with poisoned spares"""
    hip = conv_tuning
    hip.call('sn_conv_tune', cfg)
    N, C, H, W, O, K = 2, 72, 5, 7, 128, 3
    rs = np.random.RandomState(3)
    x = f16r(rs.standard_normal((N, C, H, W)))
    w = f16r(rs.standard_normal((O, C, K, K)) / np.sqrt(C * K * K))
    b = rs.standard_normal(O).astype(np.float32)
    want = Fnn.relu(Fnn.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), 1, 1, 1)).numpy()
    wd = torch.from_numpy(w_to_otI(w)).to(dev()).half().contiguous()
    bd = torch.from_numpy(b).to(dev())
    outs = []
    for ps, spare in ((C, 0.0), (80, 60000.0), (80, float('nan'))):
        xd = torch.full((N, H, W, ps), spare, dtype=torch.float16, device=dev())
        xd[..., :C] = to_nhwc_f16(x)
        y = torch.full((N, H, W, O), 777.0, dtype=torch.float16, device=dev())
        hip.call('sn_conv_fwd', xd, wd, bd, None, y, N, H, W, C, ps, O, O, 0, K, K, 1, 1, 1, 1, 0, hip.stream())      # untraced
        torch.cuda.synchronize()
        y2 = torch.full((N, H, W, O), 777.0, dtype=torch.float16, device=dev())
        st = _Stamps()
        with st:
            hip.call('sn_conv_fwd', xd, wd, bd, None, y2, N, H, W, C, ps, O, O, 0, K, K, 1, 1, 1, 1, 0, hip.stream())
        assert st.pipelined and torch.equal(y.view(torch.int16), y2.view(torch.int16))
        assert_close(from_nhwc(y), want, 1e-2, 1e-2 * np.abs(want).max(), 'ragged fwd cfg %d stride %d spare %s' % (cfg, ps, spare))
        outs.append(y)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and torch.equal(outs[0].view(torch.int16), outs[2].view(torch.int16))


# the ragged data gradients of the R101 training step at the benchmark's batch (20 chips of 32 x 32 trunk pixels, 6000 RoIs):
# N, H, W, dx channels, contraction, K, pad, dilation
R101_RAGGED = [(20, 32, 32, 512, 72, 3, 2, 2),        # the three deformable offset layers
               (20, 32, 32, 512, 48, 1, 0, 1),        # rpn_cls_score
               (20, 32, 32, 512, 88, 1, 0, 1),        # rpn_bbox_pred
               (6000, 1, 1, 1024, 88, 1, 0, 1),       # cls_score (81 classes, stored as 88)
               (6000, 1, 1, 1024, 8, 1, 0, 1),        # bbox_pred
               (6000, 1, 1, 12544, 104, 1, 0, 1)]     # the offset FullyConnected of the deformable RoI pooling (98, stored as 104)


def _launch_only(N, H, W, C, O, K, pad, dil):
    hip = _hip()
    dy = torch.zeros((N, H, W, O), dtype=torch.float16, device=dev())
    wT = torch.zeros((C, K * K, O), dtype=torch.float16, device=dev())
    dx = torch.empty((N, H, W, C), dtype=torch.float16, device=dev())
    st = _Stamps()
    with st:
        hip.call('sn_conv_dgrad', dy, wT, None, dx, N, H, W, C, C, O, O, C, K, K, 1, pad, dil, 0, hip.stream())
    return st.pipelined


@pytest.mark.parametrize('shape', R101_RAGGED)
def test_r101_ragged_data_gradients_take_the_pipeline(shape, conv_tuning):
    assert _launch_only(*shape), shape


def test_narrow_outputs_stay_on_the_register_staged_kernel(conv_tuning):
    """Nout <= 64 never takes the pipeline, ragged or not (profiles/r06_ab_nout64.txt)"""
    assert not _launch_only(2, 16, 16, 64, 72, 3, 1, 1)
    assert not _launch_only(2, 16, 16, 64, 64, 3, 1, 1)
    assert _launch_only(2, 16, 16, 72, 72, 3, 1, 1)


def test_packed_stem_stays_on_the_register_staged_kernel(conv_tuning):
    """sn_conv_stem_fwd with 128 output channels: Cin = 4 * KWP = 32 is a ragged multiple of 8 and Nout > 64, but the packed rows
    (pixel stride 4 halves) are not 16-byte addressable per pixel -- the plan's in_ps % 8 guard keeps it on conv_igemm_kernel"""
    hip = _hip()
    rs = np.random.RandomState(1)
    N, H, W, O = 1, 32, 32, 128
    x = (rs.standard_normal((N, 3, H, W)) * 50).astype(np.float32)
    w = (rs.standard_normal((O, 3, 7, 7)) / np.sqrt(147)).astype(np.float32)
    one, zero = torch.ones(3, device=dev()), torch.zeros(3, device=dev())
    Hp, Wp = H + 6, W + 8
    xp = torch.empty((N, Hp, Wp, 4), dtype=torch.float16, device=dev())
    hip.call('sn_pack_stem_input', torch.from_numpy(x).to(dev()), xp, N, 3, H, W, Hp, Wp, 3, 3, one, zero, hip.stream())
    wk = np.zeros((O, 7, 8, 4), np.float32)
    wk[:, :, :7, :3] = w.transpose(0, 2, 3, 1)
    wd = torch.from_numpy(wk.reshape(O, 7, 32)).to(dev()).half().contiguous()
    Ho, Wo = H // 2, W // 2
    y = torch.empty((N, Ho, Wo, O), dtype=torch.float16, device=dev())
    st = _Stamps()
    with st:
        hip.call('sn_conv_stem_fwd', xp, wd, None, y, N, Hp, Wp, Ho, Wo, O, O, 7, 8, 2, 0, 0, hip.stream())
    assert not st.pipelined
    want = Fnn.conv2d(torch.from_numpy(f16r(x)), torch.from_numpy(f16r(w)), None, 2, 3).numpy()
    assert_close(from_nhwc(y), want, 1e-2, 1e-2 * np.abs(want).max(), 'stem conv, 128 channels')


@pytest.mark.parametrize('O,ps', [(72, 76), (72, 84), (42, 42), (44, 48)])
def test_rows_or_taps_that_are_not_16_byte_addressable_are_refused(O, ps, conv_tuning):
    """a contraction that is no multiple of 8 channels (42 channels at pixel stride 42, 44 at 48) or a ragged one whose rows are not
    16-byte addressable (72 at stride 76 / 84) reaches neither kernel: the entry refuses it before any launch (conv_check), as it
    always did -- nothing is stamped and dx keeps its fill value"""
    from sniper_amd._lib import SniperHipError
    hip = _hip()
    N, H, W, C, K = 2, 5, 7, 128, 1
    dy = torch.zeros((N, H, W, ps), dtype=torch.float16, device=dev())
    wT = torch.zeros((C, K * K, O), dtype=torch.float16, device=dev())
    dx = torch.full((N, H, W, C), 777.0, dtype=torch.float16, device=dev())
    st = _Stamps()
    with st:
        with pytest.raises(SniperHipError) as e:
            hip.call('sn_conv_dgrad', dy, wT, None, dx, N, H, W, C, C, O, ps, C, K, K, 1, 0, 1, 0, hip.stream())
    assert 'multiple of 8' in str(e.value)
    assert not st.pipelined and bool((dx == 777.0).all().item())
