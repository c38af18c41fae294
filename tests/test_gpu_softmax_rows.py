"""-m gpu: SoftmaxOutput over contiguous rows (inner == 1: the R-CNN classifier) and the valid-label count.

The row kernels (softmax_rows_fwd_kernel / softmax_rows_bwd_kernel, nn_ops.hip) stage a block of rows through LDS and run the
statements of the strided kernels in the same order, so their results must be BIT-IDENTICAL to the strided kernels, which the
debug option `softmax_strided` selects.  Both are also held to the tolerance of test_gpu_nn_ops.py's softmax test against
torch-CPU fp32 (the reference oracle/nn.py names for the standard ops).  Row counts leave the last row block partial."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import assert_close, dev  # noqa: E402

# a block of >= 16 rows of pitch K | 1 floats in 64 KB of LDS: K <= 1023 takes the row kernels, K = 1024 the strided ones.  Which
# kernel a call took is not observable through the C ABI (the results are the same bits, which is the point): for K = 1024 the
# bitwise comparison below holds trivially, and a row path that never ran would pass it too.  What shows the dispatch is the kernel
# statistics of a profiled run (profiles/softmax_rows_ab.txt: softmax_rows_fwd_kernel / softmax_rows_bwd_kernel replace the strided
# kernels' R-CNN launches); here every K <= 1023 case is ALSO held to the torch reference, so a wrong row kernel cannot hide.
ROW_PATH_MAX_K = 1023
SHAPES = [(1, 81), (70, 81), (257, 81), (64, 2), (5, 300), (37, ROW_PATH_MAX_K), (37, ROW_PATH_MAX_K + 1)]


def _hip():
    from sniper_amd import hip
    return hip


def _labels(rs, outer, K, mode):
    lab = rs.randint(0, K, size=outer).astype(np.float32)
    if mode == 'some_ignored':
        lab[rs.rand(outer) < 0.4] = -1.0
        lab[0] = -1.0
    elif mode == 'all_ignored':
        lab[:] = -1.0
    return lab


def _run(x, lab, use_ignore, normalize_valid, strided):
    hip = _hip()
    outer, K = x.shape
    xd, ld = torch.from_numpy(x).to(dev()), torch.from_numpy(lab).to(dev())
    p, g = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    ws = torch.full((4,), 12345, dtype=torch.int32, device=dev())
    hip.call('sn_debug_option', b'softmax_strided', 1 if strided else 0)
    try:
        hip.call('sn_softmax_fwd', xd, p, outer, K, 1, hip.stream())
        hip.call('sn_softmax_output_bwd', p, ld, g, outer, K, 1, -1.0, use_ignore, 2.0, normalize_valid, ws, hip.stream())
        torch.cuda.synchronize()
    finally:
        hip.call('sn_debug_option', b'softmax_strided', 0)
    return p.cpu().numpy(), g.cpu().numpy(), int(ws[0].item())


@pytest.mark.parametrize('outer,K', SHAPES)
@pytest.mark.parametrize('mode', ['none_ignored', 'some_ignored', 'all_ignored'])
def test_softmax_rows_bitwise_and_reference(outer, K, mode):
    rs = np.random.RandomState(outer * 1000 + K)
    x = (rs.standard_normal((outer, K)) * 3).astype(np.float32)
    lab = _labels(rs, outer, K, mode)
    pt = torch.softmax(torch.from_numpy(x), 1).numpy()
    valid = lab != -1.0
    oh = np.zeros_like(x)
    oh[np.arange(outer)[valid], lab[valid].astype(int)] = 1
    for use_ignore, normalize_valid in ((1, 1), (1, 0), (0, 1)):
        p_new, g_new, c_new = _run(x, lab, use_ignore, normalize_valid, strided=False)
        p_old, g_old, c_old = _run(x, lab, use_ignore, normalize_valid, strided=True)
        what = 'softmax rows (%d,%d) %s use_ignore=%d normalize_valid=%d' % (outer, K, mode, use_ignore, normalize_valid)
        assert np.array_equal(p_new.view(np.uint32), p_old.view(np.uint32)), what + ': forward differs from the strided kernel'
        assert np.array_equal(g_new.view(np.uint32), g_old.view(np.uint32)), what + ': backward differs from the strided kernel'
        assert_close(p_new, pt, 1e-5, 1e-6, what + ' fwd')
        if use_ignore:
            count = int(valid.sum())
            want = (pt - oh) * valid[:, None]
        else:                      # label -1 matches no class: every row counts and none gets its one-hot
            count = outer
            want = pt - oh
        if normalize_valid:
            assert c_new == count and c_old == count, (what, c_new, c_old, count)      # (all ignored: 0, the kernel divides by 1)
        want = want * np.float32(2.0 / max(1, count) if normalize_valid else 2.0)
        assert_close(g_new, want, 1e-4, 1e-6, what + ' bwd')


@pytest.mark.parametrize('n', [1, 63, 64, 65, 256 * 300 + 7])
@pytest.mark.parametrize('use_ignore', [0, 1])
def test_count_valid_exact(n, use_ignore):
    """the count sn_softmax_output_bwd leaves in its workspace word (one atomicAdd per workgroup, capped grid) against numpy"""
    hip = _hip()
    rs = np.random.RandomState(n)
    lab = rs.choice([-1.0, 0.0, 1.0], size=n, p=[0.6, 0.3, 0.1]).astype(np.float32)
    p = torch.full((1, 2, n), 0.5, device=dev())
    g = torch.empty_like(p)
    ws = torch.full((4,), -99, dtype=torch.int32, device=dev())
    hip.call('sn_softmax_output_bwd', p, torch.from_numpy(lab).to(dev()), g, 1, 2, n, -1.0, use_ignore, 1.0, 1, ws, hip.stream())
    torch.cuda.synchronize()
    assert int(ws[0].item()) == (int((lab != -1.0).sum()) if use_ignore else n)
