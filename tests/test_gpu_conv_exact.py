"""-m gpu: the convolution family against the float64 reference ON THE BITS (conv_exact_util.py; DESIGN.md "Exact convolution
tests").  Integer operands make every product and partial sum exact in fp32 and every stored fp16 value exact, so a forced tile
configuration, a split, a slab order or a reduce cannot change the result: one dropped or doubled 8-channel chunk, a padding pixel
read instead of zero-filled, a unit counted twice or a residual rounded before the add is a mismatch, not noise under a tolerance.
The cases walk M, Cout and the contraction over the tile edges (conv_exact_util.cases()); every operand lives in a guarded
buffer (NaN around inputs, a sentinel around outputs that must survive the launch) at dense and padded pitches and as a channel
slice of a wider buffer."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

pytestmark = pytest.mark.gpu

import conv_exact_util as cx  # noqa: E402
from conv_exact_util import Guarded, rows_nhwc  # noqa: E402
from gpu_util import Stamps, dev  # noqa: E402

CFGS = (-1, 0, 4, 5, 6, 7, 14, 16, 18)
STATS_CFGS = (-1, 5, 6, 14, 16, 18)
# row x column tile of a configuration (csrc/conv_dma_kernel.h kCfg); -1: the built-in choice for launches of fewer than 8192 rows
# and fewer than 1024 output channels is the 64 x 128 tile (conv_dma_choice_balanced)
TILES = {-1: (64, 128), 4: (128, 256), 5: (64, 128), 6: (64, 128), 7: (256, 256), 14: (160, 128), 16: (160, 128), 18: (160, 128)}
WGRAD_MODES = ((1, 0), (1, 2), (1, 7), (1, 1000), (0, 0), (1, 100002), (1, 200002), (1, 100000 + 1000), (1, 200000 + 1000))


def _hip():
    from sniper_amd import hip
    return hip


@pytest.fixture
def conv_state():
    """the process-wide kernel-selection hooks go back to production behaviour whatever the test did"""
    hip = _hip()
    yield hip
    hip.call('sn_conv_tune', -1)
    hip.call('sn_conv_wgrad_impl', 1, 0)
    hip.call('sn_conv_dgrad_by_class', 1)
    hip.call('sn_conv_trace', None)


class _Counts(dict):
    def add(self, key, n=1):
        self[key] = self.get(key, 0) + n

    def log(self, test):
        """one JSON line per test -- cases, launches compared, pipelined / register-staged pairs -- appended to the file that
        SNIPER_TEST_COUNTS names (unset: nothing is written)"""
        path = os.environ.get('SNIPER_TEST_COUNTS')
        if not path:
            return
        try:
            with open(path, 'a') as fh:
                fh.write(json.dumps(dict(self, test=test)) + '\n')
        except OSError:
            pass


def _tile(cfg, nout, contraction, dgrad, pipelined):
    """the tile a launch ran on, for the failure message"""
    if not pipelined:
        return (128, 64 if nout <= 64 else 128)
    if contraction % 64:      # the RAGGED instantiations: 64 x 128 for 4 / 5 / 6 (and the built-in choice here), else 160 x 128
        return (64, 128) if cfg in (-1, 4, 5, 6) else (160, 128)
    return TILES[cfg]


def _kinds(i, k):
    """pitch kind of operand k of case i: every case meets every kind on some operand, every operand meets every kind on some case"""
    return cx.PITCHES[(i + k) % len(cx.PITCHES)]


def _out_kind(i, k, C):
    """... outputs of a width that is no multiple of 8 also come exactly packed (rows that are not 16-byte aligned)"""
    if C % 8 and (i + k) % 3 == 0:
        return 'packed'
    return _kinds(i, k)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _check_out(buf, want_rows, what, row_len, rows_img, tile):
    cx.assert_exact_rows(buf.result(), want_rows, what, row_len, rows_img, tile)
    assert buf.untouched(), '%s: the launch wrote outside its %d x %d output (pitch %d, offset %d)' % (what, buf.rows, buf.C, buf.pitch, buf.offset)


# ------------------------------------------------------------------------------------------------------------------ sn_conv_fwd
def _fwd_modes(q, i):
    """(name, bias, residual rows, relu, out_f32, want rows)"""
    return (('plain', None, None, 0, 0, rows_nhwc(q.y)),
            ('bias+res+relu', q.bias, rows_nhwc(q.res), 1, 0, rows_nhwc(q.y_brr)),
            ('f32 quarter bias', q.bias_q, None, 0, 1, rows_nhwc(q.y_q)))


@pytest.mark.parametrize('cfg', CFGS)
def test_conv_fwd_exact(cfg, conv_state):
    hip = conv_state
    hip.call('sn_conv_tune', cfg)
    st = Stamps(words=1 << 14)
    n = _Counts()
    for i, case in enumerate(cx.cases()):
        N, H, W, C, O, K, s, p, d = case
        q = cx.problem(case)
        Ho, Wo, M = cx.case_dims(case)
        x = Guarded(N * H * W, C, _kinds(i, 0), values=rows_nhwc(q.x))
        w = Guarded(O, K * K * C, 'dense', values=cx.w_rows(q.w))
        want_pipe = cfg != 0 and O >= 65        # (C % 8 == 0 and 16-byte pitches throughout: conv_plan's whole rule for plain launches)
        for k, (mode, bias, res, relu, f32, want) in enumerate(_fwd_modes(q, i)):
            what = 'sn_conv_fwd %s case %s cfg %d' % (mode, case, cfg)
            b = _f32(bias) if bias is not None else None
            r = Guarded(M, O, _kinds(i, 2 + k), values=res) if res is not None else None
            outs = []
            for traced in (False, True):
                y = Guarded(M, O, _out_kind(i, 1 + k, O), dtype=torch.float32 if f32 else torch.float16)
                args = (x.view, w.view, b, r.view if r else None, y.view, N, H, W, C, x.pitch, O, y.pitch, r.pitch if r else 0, K, K, s, p, d,
                        relu, f32, hip.stream())
                if traced:
                    with st:
                        hip.call('sn_conv_fwd', *args)
                    assert st.pipelined == want_pipe, '%s: %s kernel ran' % (what, 'the pipelined' if st.pipelined else 'the register-staged')
                else:
                    hip.call('sn_conv_fwd', *args)
                outs.append(y)
            got = outs[0].result()
            assert np.array_equal(got.view(np.int32 if f32 else np.int16), outs[1].result().view(np.int32 if f32 else np.int16)), what + ': traced run differs'
            for y in outs:
                _check_out(y, want, what, Wo, Ho * Wo, _tile(cfg, O, C, False, want_pipe))
            n.add('launches', 2)
        n.add('cases')
        n.add('pipelined' if want_pipe else 'register_staged')
    n.log('fwd cfg %d' % cfg)


# ---------------------------------------------------------------------------------------------------------------- sn_conv_dgrad
def _transposed_weights(hip, q, Op):
    """the data gradient's weight copy through sn_weight_transpose, as the engine makes it; itself checked bit for bit"""
    N, H, W, C, O, K, s, p, d = q.case
    wT = Guarded(C, K * K * Op, 'dense')
    hip.call('sn_weight_transpose', _f32(cx.w_rows(q.w)), wT.view, O, K * K, C, Op, hip.stream())
    cx.assert_exact_rows(wT.result(), cx.wt_rows(q.w, Op), 'sn_weight_transpose case %s' % (q.case,))
    keep = wT.view.clone()
    assert wT.untouched(), 'sn_weight_transpose wrote outside [Cin][taps][O_pad], case %s' % (q.case,)
    wT.view.copy_(keep)
    wT.flat[:cx.GUARD_ROWS * wT.pitch] = float('nan')          # as an input: NaN guards
    wT.flat[(cx.GUARD_ROWS + wT.rows) * wT.pitch:] = float('nan')
    return wT


@pytest.mark.parametrize('cfg', CFGS)
def test_conv_dgrad_exact(cfg, conv_state):
    hip = conv_state
    hip.call('sn_conv_tune', cfg)
    st = Stamps(words=1 << 14)
    n = _Counts()
    for i, case in enumerate(cx.cases()):
        N, H, W, C, O, K, s, p, d = case
        q = cx.problem(case)
        Ho, Wo, M = cx.case_dims(case)
        Op = (O + 7) // 8 * 8                  # the contraction: dy and the transposed weights carry zeros in lanes [O, Op)
        dy = Guarded(M, O, _kinds(i, 0), values=rows_nhwc(q.dy), zero_to=Op)
        wT = _transposed_weights(hip, q, Op)
        want_pipe = cfg != 0 and C >= 65
        tile = _tile(cfg, C, Op, True, want_pipe)
        rows = N * H * W
        for by_class in ((1, 0) if s == 2 else (1,)):
            hip.call('sn_conv_dgrad_by_class', by_class)
            for k, (mode, acc, f32, want) in enumerate((('plain', None, 0, rows_nhwc(q.dx)), ('accumulate', 'own', 0, rows_nhwc(q.dx_acc)),
                                                      ('accumulate in place', 'alias', 0, rows_nhwc(q.dx_acc)), ('f32', None, 1, rows_nhwc(q.dx)))):
                what = 'sn_conv_dgrad %s case %s cfg %d by_class %d' % (mode, case, cfg, by_class)
                a = Guarded(rows, C, _kinds(i, 2 + k), values=rows_nhwc(q.acc)) if acc == 'own' else None
                outs = []
                for traced in (False, True):
                    dx = Guarded(rows, C, _out_kind(i, 1 + k, C), dtype=torch.float32 if f32 else torch.float16)
                    if acc == 'alias':
                        dx.view.copy_(torch.from_numpy(rows_nhwc(q.acc)).to(dev()))
                    av, aps = (a.view, a.pitch) if a else ((dx.view, dx.pitch) if acc == 'alias' else (None, 0))
                    args = (dy.view, wT.view, av, dx.view, N, H, W, C, dx.pitch, Op, dy.pitch, aps, K, K, s, p, d, f32, hip.stream())
                    if traced:
                        with st:
                            hip.call('sn_conv_dgrad', *args)
                        assert st.pipelined == want_pipe, '%s: %s kernel ran' % (what, 'the pipelined' if st.pipelined else 'the register-staged')
                    else:
                        hip.call('sn_conv_dgrad', *args)
                    outs.append(dx)
                bits = np.int32 if f32 else np.int16
                assert np.array_equal(outs[0].result().view(bits), outs[1].result().view(bits)), what + ': traced run differs'
                for dx in outs:
                    _check_out(dx, want, what, W, H * W, tile)
                n.add('launches', 2)
        n.add('cases')
        n.add('pipelined' if want_pipe else 'register_staged')
    n.log('dgrad cfg %d' % cfg)


# ------------------------------------------------------------------------------------------- sn_conv_fwd_stats / sn_conv_dgrad_bn
def _check_partials(part, blocks, per_row, bm, what, in_order=True):
    """partials (blocks, 2, C) fp32 against the float64 sums of `per_row` = (rows of the first sum, rows of the second): the totals
    always; each block's row when the rows run in order (`in_order`: not the parity-class walk)"""
    got = part.result().astype(np.float64).reshape(blocks, 2, -1)
    M = per_row[0].shape[0]
    for which in (0, 1):
        assert np.abs(per_row[which]).sum(axis=0).max() < cx.FP32_EXACT, what          # exact in fp32 in any order
        if in_order:
            assert blocks == -(-M // bm), what
            want = cx.block_sums(per_row[which], bm)
            bad = cx.first_mismatch(got[:, which], want)
            assert bad is None, '%s: sum %d of row tile %d (rows %d..), channel %d: got %r want %r' % (
                what, which, bad[0], bad[0] * bm, bad[1], got[bad[0], which, bad[1]], want[bad])
        total, want_t = got[:, which].sum(axis=0), per_row[which].sum(axis=0)
        assert np.array_equal(total, want_t), '%s: sum %d over all blocks, channel %d: got %r want %r' % (
            what, which, int(np.argmax(total != want_t)), total[np.argmax(total != want_t)], want_t[np.argmax(total != want_t)])
    assert part.untouched(), what + ': wrote outside the partials'


@pytest.mark.parametrize('cfg', STATS_CFGS)
def test_conv_fwd_stats_exact(cfg, conv_state):
    """y bit-equal to the reference and the per-row-tile sum / sum of squares of the STORED values equal to the float64 sums"""
    hip = conv_state
    hip.call('sn_conv_tune', cfg)
    n = _Counts()
    for i, case in enumerate(cx.cases()):
        N, H, W, C, O, K, s, p, d = case
        Ho, Wo, M = cx.case_dims(case)
        kx, ky, kr = _kinds(i, 0), _kinds(i, 1), _kinds(i, 2)
        xp, yp, rp = cx.pitch_of(C, kx)[0], cx.pitch_of(O, ky)[0], cx.pitch_of(O, kr)[0]
        for mode in ('plain', 'bias+res+relu'):
            rps = rp if mode != 'plain' else 0
            blocks = hip.query('sn_conv_fwd_stats_blocks', N, H, W, C, xp, O, yp, rps, K, K, s, p, d)
            assert (blocks > 0) == (O >= 65 and O % 4 == 0 and C % 64 == 0), (case, cfg, blocks)
            if blocks <= 0:
                continue
            bm = TILES[cfg][0]
            assert blocks == -(-M // bm), (case, cfg, blocks, bm)
            q = cx.problem(case)
            what = 'sn_conv_fwd_stats %s case %s cfg %d' % (mode, case, cfg)
            x = Guarded(N * H * W, C, kx, values=rows_nhwc(q.x))
            w = Guarded(O, K * K * C, 'dense', values=cx.w_rows(q.w))
            r = Guarded(M, O, kr, values=rows_nhwc(q.res)) if rps else None
            y = Guarded(M, O, ky)
            part = Guarded(blocks * 2, O, 'packed', dtype=torch.float32)
            hip.call('sn_conv_fwd_stats', x.view, w.view, _f32(q.bias) if rps else None, r.view if r else None, y.view, N, H, W, C, x.pitch, O,
                     y.pitch, rps, K, K, s, p, d, 1 if rps else 0, part.view, hip.stream())
            want = rows_nhwc(q.y_brr if rps else q.y)
            assert 256 * np.abs(want).max() ** 2 < cx.FP32_EXACT
            _check_out(y, want, what, Wo, Ho * Wo, TILES[cfg])
            _check_partials(part, blocks, (want, want * want), bm, what)
            n.add('launches')
        n.add('cases')
    assert n.get('launches', 0) >= 20, n
    n.log('fwd_stats cfg %d' % cfg)


@pytest.mark.parametrize('cfg', STATS_CFGS)
def test_conv_dgrad_bn_exact(cfg, conv_state):
    """dx bit-equal to the reference and the per-row-tile sum g / sum g (bn_x - mean) equal to the float64 sums, for no activation,
    ReLU and ReLU6; the stride-2 cases under the parity-class walk (totals) and the every-tap walk (block by block)"""
    hip = conv_state
    hip.call('sn_conv_tune', cfg)
    n = _Counts()
    for i, case in enumerate(cx.cases()):
        N, H, W, C, O, K, s, p, d = case
        Ho, Wo, M = cx.case_dims(case)
        Op = (O + 7) // 8 * 8
        kdy, kdx, kbx = _kinds(i, 0), _kinds(i, 1), _kinds(i, 3)
        dyp, dxp = cx.pitch_of(Op, kdy)[0], cx.pitch_of(C, kdx)[0]
        rows = N * H * W
        for by_class in ((1, 0) if s == 2 else (1,)):
            hip.call('sn_conv_dgrad_by_class', by_class)
            blocks = hip.query('sn_conv_dgrad_bn_blocks', N, H, W, C, dxp, Op, dyp, 0, K, K, s, p, d)
            assert (blocks > 0) == (C >= 65 and C % 4 == 0 and Op % 64 == 0), (case, cfg, blocks)
            if blocks <= 0:
                continue
            bm = TILES[cfg][0]
            classes = s == 2 and d == 1 and H % 2 == 0 and W % 2 == 0 and by_class == 1 and cfg != 18
            assert blocks == (4 * -(-(rows // 4) // bm) if classes else -(-rows // bm)), (case, cfg, by_class, blocks)
            q = cx.problem(case)
            dy = Guarded(M, O, kdy, values=rows_nhwc(q.dy), zero_to=Op)
            wT = _transposed_weights(hip, q, Op)
            bx = Guarded(rows, C, kbx, values=rows_nhwc(q.bn_x))
            sc, sh, mu = _f32(q.bn_scale), _f32(q.bn_shift), _f32(q.bn_mean)
            for act in (0, 1, 2):
                what = 'sn_conv_dgrad_bn act %d case %s cfg %d by_class %d' % (act, case, cfg, by_class)
                dx = Guarded(rows, C, kdx)
                part = Guarded(blocks * 2, C, 'packed', dtype=torch.float32)
                hip.call('sn_conv_dgrad_bn', dy.view, wT.view, None, dx.view, N, H, W, C, dx.pitch, Op, dy.pitch, 0, K, K, s, p, d, bx.view,
                         bx.pitch, sc, sh, mu, act, part.view, hip.stream())
                want = rows_nhwc(q.dx)
                _check_out(dx, want, what, W, H * W, TILES[cfg])
                g = want * cx.bn_mask(rows_nhwc(q.bn_x), q.bn_scale, q.bn_shift, act)
                _check_partials(part, blocks, (g, g * (rows_nhwc(q.bn_x) - q.bn_mean)), bm, what, in_order=not classes)
                n.add('launches')
            n.add('class_walk' if classes else 'row_walk')
        n.add('cases')
    assert n.get('launches', 0) >= 20 and n.get('row_walk', 0) > 0 and (cfg == 18 or n.get('class_walk', 0) > 0), n
    n.log('dgrad_bn cfg %d' % cfg)


# ------------------------------------------------------------------------------- sn_conv_fwd_splitk / _splitk_f32 / sn_conv_fwd_dual
def _splitk_shapes(hip):
    """the four smallest shapes of test_conv_fwd_splitk_equals_plain_forward that split, and two of the same form with ragged M and
    a last column tile of 8 channels: (N, C, H, W, O, K, pad, dil, bias, residual, relu)"""
    from test_gpu_nn_ops import test_conv_fwd_splitk_equals_plain_forward as theirs
    shapes = [m for m in theirs.pytestmark if m.name == 'parametrize'][0].args[1]
    split = [t[:11] for t in shapes
             if hip.query('sn_conv_fwd_splitk_workspace_bytes', t[0], t[2], t[3], t[1], t[1], t[4], t[4], t[4] if t[9] else 0, t[5], t[5], 1, t[6], t[7]) > 0]
    split.sort(key=lambda t: t[0] * t[2] * t[3] * t[1] * t[4] * t[5] ** 2)
    return split[:4] + [(2, 512, 35, 37, 136, 3, 1, 1, True, True, 1), (3, 1024, 19, 23, 264, 1, 0, 1, True, False, 0)]


@pytest.mark.parametrize('which', range(6))
def test_conv_fwd_splitk_and_dual_exact(which, conv_state):
    hip = conv_state
    N, C, H, W, O, K, p, d, hb, hr, relu = _splitk_shapes(hip)[which]
    case = (N, H, W, C, O, K, 1, p, d)
    q = cx.problem(case, False)
    M = N * H * W
    what = 'case %s' % (case,)
    x = Guarded(M, C, 'dense', values=rows_nhwc(q.x))
    w = Guarded(O, K * K * C, 'dense', values=cx.w_rows(q.w))
    b = _f32(q.bias) if hb else None
    r = Guarded(M, O, '+8', values=rows_nhwc(q.res)) if hr else None
    rps = r.pitch if r else 0
    pre = q.y + (q.bias.reshape(1, O, 1, 1) if hb else 0.0) + (q.res if hr else 0.0)
    want = rows_nhwc(np.maximum(pre, 0.0) if relu else pre)
    assert np.abs(want).max() <= cx.FP16_EXACT
    ykind = 'dense' if O % 8 else '+24'
    y = Guarded(M, O, ykind)
    geom = (N, H, W, C, x.pitch, O, y.pitch, rps, K, K, 1, p, d)
    need = hip.query('sn_conv_fwd_splitk_workspace_bytes', *geom)
    assert need > 0, (case, need)
    ws = torch.full((need,), 0x7f, dtype=torch.uint8, device=dev())
    hip.call('sn_conv_fwd_splitk', x.view, w.view, b, r.view if r else None, y.view, *geom, relu, ws, need, hip.stream())
    _check_out(y, want, 'sn_conv_fwd_splitk ' + what, W, H * W, (64, 128))
    if not hr:
        ws.fill_(0x7f)
        yf = Guarded(M, O, ykind, dtype=torch.float32)
        hip.call('sn_conv_fwd_splitk_f32', x.view, w.view, b, yf.view, N, H, W, C, x.pitch, O, yf.pitch, K, K, 1, p, d, relu, ws, need, hip.stream())
        _check_out(yf, want, 'sn_conv_fwd_splitk_f32 ' + what, W, H * W, (64, 128))
    # the second output y2 = act(y2_scale * y + y2_shift) of the stored y, with its own pitch: split (scratch) and unsplit (none)
    rs = np.random.RandomState(cx.case_seed(case, 99))
    s2, t2 = rs.choice([0.5, 1.0, 2.0], size=O), rs.randint(-8, 9, size=O).astype(np.float64)
    want2 = np.maximum(want * s2 + t2, 0.0)
    assert np.array_equal(want2.astype(np.float16).astype(np.float64), want2)
    ok = hip.query('sn_conv_fwd_dual_ok', *geom, cx.pitch_of(O, 'slice')[0])
    assert ok == (1 if O % 8 == 0 else 0), (case, ok)
    if ok:
        for scratch in (ws, None):
            if scratch is not None:
                ws.fill_(0x7f)
            y, y2 = Guarded(M, O, ykind), Guarded(M, O, 'slice')
            hip.call('sn_conv_fwd_dual', x.view, w.view, b, r.view if r else None, y.view, *geom, relu, y2.view, y2.pitch, _f32(s2), _f32(t2), 1,
                     scratch, need if scratch is not None else 0, hip.stream())
            tag = 'sn_conv_fwd_dual %s %s' % ('split' if scratch is not None else 'unsplit', what)
            _check_out(y, want, tag + ' y', W, H * W, (64, 128))
            _check_out(y2, want2, tag + ' y2', W, H * W, (64, 128))


def test_conv_fwd_splitk_on_the_generated_cases_exact(conv_state):
    """most of the generator's cases are too small to split: the workspace query is 0 and sn_conv_fwd_splitk is the documented
    fall-back to sn_conv_fwd (no scratch); the few long contractions on a handful of tiles that do split run with their scratch"""
    hip = conv_state
    n = _Counts()
    for i, case in enumerate(cx.cases()):
        N, H, W, C, O, K, s, p, d = case
        Ho, Wo, M = cx.case_dims(case)
        kx, kr, ky = _kinds(i, 0), _kinds(i, 2), _out_kind(i, 1, O)
        geom = (N, H, W, C, cx.pitch_of(C, kx)[0], O, cx.pitch_of(O, ky)[0], cx.pitch_of(O, kr)[0], K, K, s, p, d)
        need = hip.query('sn_conv_fwd_splitk_workspace_bytes', *geom)
        if need == 0 and i % 4:
            continue
        q = cx.problem(case)
        x = Guarded(N * H * W, C, kx, values=rows_nhwc(q.x))
        w = Guarded(O, K * K * C, 'dense', values=cx.w_rows(q.w))
        r = Guarded(M, O, kr, values=rows_nhwc(q.res))
        y = Guarded(M, O, ky)
        assert geom[4] == x.pitch and geom[6] == y.pitch and geom[7] == r.pitch
        ws = torch.full((need,), 0x7f, dtype=torch.uint8, device=dev()) if need else None
        what = '(%s) case %s' % ('split, %d bytes' % need if need else 'no split', case)
        hip.call('sn_conv_fwd_splitk', x.view, w.view, _f32(q.bias), r.view, y.view, *geom, 1, ws, need, hip.stream())
        _check_out(y, rows_nhwc(q.y_brr), 'sn_conv_fwd_splitk ' + what, Wo, Ho * Wo, (64, 128))
        if need:
            ws.fill_(0x7f)
        yf = Guarded(M, O, ky, dtype=torch.float32)
        hip.call('sn_conv_fwd_splitk_f32', x.view, w.view, _f32(q.bias_q), yf.view, N, H, W, C, x.pitch, O, yf.pitch, K, K, s, p, d, 0, ws, need,
                 hip.stream())
        _check_out(yf, rows_nhwc(q.y_q), 'sn_conv_fwd_splitk_f32 ' + what, Wo, Ho * Wo, (64, 128))
        n.add('split' if need else 'fallback')
    assert n.get('fallback', 0) >= 30 and n.get('split', 0) >= 1, n
    n.log('splitk on the generated cases')


# ----------------------------------------------------------------------------------------------------------------- weight gradient
def _dw_rows(a_oikk):
    return cx.w_rows(a_oikk)


class _WgradOperands(object):
    """dy, x of a case in guarded buffers at the case's pitches"""

    def __init__(self, i, case, x_kind=None):
        N, H, W, C, O, K, s, p, d = case
        q = cx.problem(case)
        Ho, Wo, M = cx.case_dims(case)
        self.case, self.q = case, q
        self.dy = Guarded(M, O, _kinds(i, 0), values=rows_nhwc(q.dy), zero_to=(O + 7) // 8 * 8)
        self.x = Guarded(N * H * W, C, x_kind or _kinds(i, 1), values=rows_nhwc(q.x))
        self.geom = (N, H, W, C, self.x.pitch, O, self.dy.pitch, K, K, s, p, d)

    def dw(self, start):
        N, H, W, C, O, K, s, p, d = self.case
        out = Guarded(O, K * K * C, 'packed', dtype=torch.float32)
        out.view.copy_(_f32(_dw_rows(start)))
        return out


def _check_dw(dwb, want_oikk, what, C):
    got, want = dwb.result(), _dw_rows(want_oikk)
    bad = cx.first_mismatch(got, want)
    assert bad is None, '%s: dw[co %d][tap %d][ci %d] (128 x 128 tile (%d, %d)): got %r want %r' % (
        what, bad[0], bad[1] // C, bad[1] % C, bad[0] // 128, bad[1] % C // 128, float(got[bad]), float(want[bad]))
    assert dwb.untouched(), what + ': wrote outside dw'


@pytest.mark.parametrize('mode', WGRAD_MODES)
def test_conv_wgrad_exact(mode, conv_state):
    """every job length and both forced tile heights of the batched kernel, and the gather kernel: `dw += ` on a non-zero integer dw
    with the queried scratch, and into zeros without scratch (unsplit, one owner per element) -- split order, slabs and the reduce
    cannot change an exact sum"""
    hip = conv_state
    hip.call('sn_conv_wgrad_impl', *mode)
    n = _Counts()
    for i, case in enumerate(cx.cases()):
        N, H, W, C, O, K, s, p, d = case
        op = _WgradOperands(i, case)
        q = op.q
        need = hip.query('sn_conv_wgrad_workspace_bytes', *op.geom)
        ws = torch.full((max(need, 16),), 0x7f, dtype=torch.uint8, device=dev())
        what = 'sn_conv_wgrad case %s impl %s' % (case, mode)
        dw = op.dw(q.dw0)
        hip.call('sn_conv_wgrad', op.dy.view, op.x.view, dw.view, *op.geom, ws, need, hip.stream())
        _check_dw(dw, q.dw0 + q.dw, what + ' scratch %d, dw += ' % need, C)
        dw = op.dw(np.zeros_like(q.dw))
        hip.call('sn_conv_wgrad', op.dy.view, op.x.view, dw.view, *op.geom, None, 0, hip.stream())
        _check_dw(dw, q.dw, what + ' no scratch', C)
        n.add('launches', 2)
        n.add('split' if need else 'unsplit')
    n.log('wgrad impl %s' % (mode,))


def test_conv_wgrad_unaligned_pitch_reaches_the_gather_kernel_exact(conv_state):
    """an x pitch that is no multiple of 8 halves is not 16-byte addressable: the default impl hands the layer to the gather kernel"""
    hip = conv_state
    for i, case in enumerate(cx.cases()):
        if i % 6:
            continue
        N, H, W, C, O, K, s, p, d = case
        q = cx.problem(case)
        Ho, Wo, M = cx.case_dims(case)
        dy = Guarded(M, O, _kinds(i, 0), values=rows_nhwc(q.dy), zero_to=(O + 7) // 8 * 8)
        xps = C + 4
        xf = torch.full(((2 * cx.GUARD_ROWS + N * H * W) * xps,), float('nan'), dtype=torch.float16, device=dev())
        xv = xf[cx.GUARD_ROWS * xps:(cx.GUARD_ROWS + N * H * W) * xps].view(N * H * W, xps)[:, :C]
        xv.copy_(torch.from_numpy(rows_nhwc(q.x)).to(dev()))
        geom = (N, H, W, C, xps, O, dy.pitch, K, K, s, p, d)
        need = hip.query('sn_conv_wgrad_workspace_bytes', *geom)
        ws = torch.full((max(need, 16),), 0x7f, dtype=torch.uint8, device=dev())
        dw = Guarded(O, K * K * C, 'packed', dtype=torch.float32)
        dw.view.copy_(_f32(_dw_rows(q.dw0)))
        hip.call('sn_conv_wgrad', dy.view, xv, dw.view, *geom, ws, need, hip.stream())
        _check_dw(dw, q.dw0 + q.dw, 'sn_conv_wgrad, x pitch %d, case %s' % (xps, case), C)


def _interleaved_cases():
    """(index, case) with narrow (Cout <= 128) and wide layers alternating: a table holds both passes of the batched launch"""
    cs = list(enumerate(cx.cases()))
    narrow, wide = [t for t in cs if t[1][4] <= 128], [t for t in cs if t[1][4] > 128]
    out = []
    while narrow or wide:
        if narrow:
            out.append(narrow.pop(0))
        if wide:
            out.append(wide.pop(0))
    return out


@pytest.mark.parametrize('table', [1, 24, 25, 60])
def test_conv_wgrad_batch_exact(table, conv_state):
    """tables of 1, 24, 25 and 60 layers (the 24-problem chunk cut, both tile-height passes) with full scratch (dw += on non-zero
    dw), scratch one byte short of the query (the documented unsplit path) and none: every dw against the float64 reference"""
    hip = conv_state
    ops = [_WgradOperands(i, case) for i, case in _interleaved_cases()]
    n = _Counts()
    for t0 in range(0, len(ops), table):
        chunk = ops[t0:t0 + table]
        for cond in ('full', 'short', 'none'):
            dws = [o.dw(o.q.dw0 if cond == 'full' else np.zeros_like(o.q.dw)) for o in chunk]
            tab = hip.wgrad_table([(o.dy.view, o.x.view, dwb.view) + o.geom for o, dwb in zip(chunk, dws)])
            need = hip.query('sn_conv_wgrad_batch_workspace_bytes', tab, len(chunk))
            if cond == 'short' and need == 0:
                continue
            ws = torch.full((max(need, 16),), 0x7f, dtype=torch.uint8, device=dev())
            if cond == 'full':
                hip.call('sn_conv_wgrad_batch', tab, len(chunk), ws, need, hip.stream())
            elif cond == 'short':
                hip.call('sn_conv_wgrad_batch', tab, len(chunk), ws, need - 1, hip.stream())
            else:
                hip.call('sn_conv_wgrad_batch', tab, len(chunk), None, 0, hip.stream())
            for o, dwb in zip(chunk, dws):
                _check_dw(dwb, (o.q.dw0 + o.q.dw) if cond == 'full' else o.q.dw,
                          'sn_conv_wgrad_batch table of %d from %d, scratch %s (%d bytes), case %s' % (len(chunk), t0, cond, need, o.case), o.case[3])
            n.add('launches')
            n.add('problems', len(chunk))
    n.log('wgrad_batch table %d' % table)


# ------------------------------------------------------------------------------------------------------------------- the siblings
def _gconv_shapes():
    from test_gpu_gconv import _FAST, _PLAIN
    return _FAST + _PLAIN


def test_gconv_exact(conv_state):
    hip = conv_state
    for i, (N, C, O, g, H, W, K, s, p, d, extra) in enumerate(_gconv_shapes()):
        q = cx.grouped_problem(N, C, O, g, H, W, K, s, p, d)
        Ho, Wo = cx.out_dim(H, K, s, p, d), cx.out_dim(W, K, s, p, d)
        M, Cg = N * Ho * Wo, C // g
        what = 'case %s' % (q.case,)
        okind = '+24' if extra == 24 else ('+8' if extra == 8 else _kinds(i, 1))
        x = Guarded(N * H * W, C, _kinds(i, 0), values=rows_nhwc(q.x))
        w = Guarded(O, K * K * Cg, 'packed', values=cx.w_rows(q.w))
        for bias, relu, want in ((None, 0, q.y), (q.bias, 1, q.y_br)):
            y = Guarded(M, O, okind)
            hip.call('sn_gconv_fwd', x.view, w.view, _f32(bias) if bias is not None else None, y.view, N, H, W, C, x.pitch, O, y.pitch, g, K, K,
                     s, p, d, relu, 0, hip.stream())
            _check_out(y, rows_nhwc(want), 'sn_gconv_fwd relu %d %s' % (relu, what), Wo, Ho * Wo, None)
        dy = Guarded(M, O, okind, values=rows_nhwc(q.dy))
        for acc in (None, 'own', 'alias'):
            dx = Guarded(N * H * W, C, _kinds(i, 2))
            a = Guarded(N * H * W, C, _kinds(i, 3), values=rows_nhwc(q.acc)) if acc == 'own' else None
            if acc == 'alias':
                dx.view.copy_(torch.from_numpy(rows_nhwc(q.acc)).to(dev()))
            av, aps = (a.view, a.pitch) if a else ((dx.view, dx.pitch) if acc else (None, 0))
            hip.call('sn_gconv_dgrad', dy.view, w.view, av, dx.view, N, H, W, C, O, dy.pitch, aps, dx.pitch, g, K, K, s, p, d, hip.stream())
            _check_out(dx, rows_nhwc(q.dx_acc if acc else q.dx), 'sn_gconv_dgrad accumulate %s %s' % (acc, what), W, H * W, None)
        need = hip.query('sn_gconv_wgrad_workspace_bytes', N, H, W, C, O, g, K, K, s, p, d)
        ws = torch.full((max(need, 16),), 0x7f, dtype=torch.uint8, device=dev())
        dw = Guarded(O, K * K * Cg, 'packed', dtype=torch.float32)
        dw.view.copy_(_f32(cx.w_rows(q.dw0)))
        hip.call('sn_gconv_wgrad', dy.view, x.view, dw.view, N, H, W, C, O, dy.pitch, x.pitch, g, K, K, s, p, d, ws, need, hip.stream())
        _check_dw(dw, q.dw0 + q.dw, 'sn_gconv_wgrad ' + what, Cg)


def _dw_shapes():
    """the four shapes of test_depthwise_conv_vs_torch (N, C, H, W, stride) with dense pitches, and two with a pitch wider than C"""
    from test_gpu_nn_ops import test_depthwise_conv_vs_torch as theirs
    shapes = [m for m in theirs.pytestmark if m.name == 'parametrize'][0].args[1]
    return [t + ('dense',) for t in shapes] + [(2, 40, 9, 11, 1, '+24'), (2, 72, 10, 7, 2, 'slice')]


def test_dwconv_exact(conv_state):
    hip = conv_state
    for (N, C, H, W, s, kind) in _dw_shapes():
        q = cx.grouped_problem(N, C, C, C, H, W, 3, s, 1, 1)
        Ho, Wo = cx.out_dim(H, 3, s, 1, 1), cx.out_dim(W, 3, s, 1, 1)
        M = N * Ho * Wo
        what = 'case %s pitch %s' % (q.case, kind)
        x = Guarded(N * H * W, C, kind, values=rows_nhwc(q.x))
        w = Guarded(C, 9, 'packed', values=q.w.reshape(C, 9))
        y = Guarded(M, C, kind)
        hip.call('sn_dwconv_fwd', x.view, w.view, y.view, N, H, W, C, x.pitch, y.pitch, 3, 3, s, 1, 1, hip.stream())
        _check_out(y, rows_nhwc(q.y), 'sn_dwconv_fwd ' + what, Wo, Ho * Wo, None)
        dy = Guarded(M, C, kind, values=rows_nhwc(q.dy))
        for acc in (None, 'own', 'alias'):
            dx = Guarded(N * H * W, C, kind)
            a = Guarded(N * H * W, C, '+8' if kind != 'dense' else 'dense', values=rows_nhwc(q.acc)) if acc == 'own' else None
            if acc == 'alias':
                dx.view.copy_(torch.from_numpy(rows_nhwc(q.acc)).to(dev()))
            av, aps = (a.view, a.pitch) if a else ((dx.view, dx.pitch) if acc else (None, 0))
            hip.call('sn_dwconv_dgrad', dy.view, w.view, av, dx.view, N, H, W, C, dy.pitch, aps, dx.pitch, 3, 3, s, 1, 1, hip.stream())
            _check_out(dx, rows_nhwc(q.dx_acc if acc else q.dx), 'sn_dwconv_dgrad accumulate %s %s' % (acc, what), W, H * W, None)
        need = hip.query('sn_dwconv_wgrad_workspace_bytes', N, H, W, C, 3, 3, s, 1, 1)
        ws = torch.full((max(need, 16),), 0x7f, dtype=torch.uint8, device=dev())
        dw = Guarded(C, 9, 'packed', dtype=torch.float32)
        dw.view.copy_(_f32(q.dw0.reshape(C, 9)))
        hip.call('sn_dwconv_wgrad', dy.view, x.view, dw.view, N, H, W, C, dy.pitch, x.pitch, 3, 3, s, 1, 1, ws, need, hip.stream())
        _check_dw(dw, (q.dw0 + q.dw).reshape(C, 1, 3, 3), 'sn_dwconv_wgrad ' + what, 1)


# the packed-stem shapes of test_conv_stem_packed_7x7 and test_stem_conv_3x3_wgrad_packed (test_gpu_nn_ops.py):
# N, H, W, O, K, stride, pad, Hp, Wp, KWP
_STEMS = [(2, 64, 64, 64, 7, 2, 3, 64 + 6, 64 + 8, 8), (2, 32, 40, 32, 3, 2, 1, 33, 42, 4)]


@pytest.mark.parametrize('shape', _STEMS)
def test_conv_stem_exact(shape, conv_state):
    """sn_conv_stem_fwd / sn_conv_stem_wgrad on the packed input (sn_pack_stem_input with scale 1, shift 0), weights packed as
    [O][KH][KWP * 4] with zeros beyond the kernel width and in channel 3"""
    hip = conv_state
    N, H, W, O, K, s, pad, Hp, Wp, KWP = shape
    rs = np.random.RandomState(cx.case_seed(shape))
    x = cx.int_operand(rs, (N, 3, H, W), -3, 3)
    w = cx.masked_weights(rs, (O, 3, K, K), 3 * K * K)
    y_ref = Fnn.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, s, pad).numpy() + 0.0
    dy = cx.int_operand(rs, y_ref.shape, -3, 3)
    dw0 = cx.int_operand(rs, (O, K, KWP, 4), -8, 8)
    assert np.abs(y_ref).max() <= cx.FP16_EXACT and float((y_ref == 0).mean()) <= cx.MAX_ZERO_SHARE
    Ho, Wo = y_ref.shape[2], y_ref.shape[3]
    assert (Ho - 1) * s + K <= Hp and (Wo - 1) * s + KWP <= Wp
    one, zero = torch.ones(3, device=dev()), torch.zeros(3, device=dev())
    xp = Guarded(N * Hp * Wp, 4, 'packed')
    hip.call('sn_pack_stem_input', _f32(x), xp.view, N, 3, H, W, Hp, Wp, pad, pad, one, zero, hip.stream())
    want_xp = np.zeros((N, Hp, Wp, 4))
    want_xp[:, pad:pad + H, pad:pad + W, :3] = x.transpose(0, 2, 3, 1)
    cx.assert_exact_rows(xp.result(), want_xp.reshape(-1, 4), 'sn_pack_stem_input %s' % (shape,))
    keep = xp.view.clone()
    assert xp.untouched()
    xp.view.copy_(keep)
    wk = np.zeros((O, K, KWP, 4))
    wk[:, :, :K, :3] = w.transpose(0, 2, 3, 1)
    wd = Guarded(O, K * KWP * 4, 'packed', values=wk.reshape(O, -1))
    for okind, f32 in (('dense', 0), ('+8', 0), ('slice', 1)):
        y = Guarded(N * Ho * Wo, O, okind, dtype=torch.float32 if f32 else torch.float16)
        hip.call('sn_conv_stem_fwd', xp.view, wd.view, None, y.view, N, Hp, Wp, Ho, Wo, O, y.pitch, K, KWP, s, 0, f32, hip.stream())
        _check_out(y, rows_nhwc(y_ref), 'sn_conv_stem_fwd %s pitch %s' % (shape, okind), Wo, Ho * Wo, (128, 64))
    need = hip.query('sn_conv_stem_wgrad_workspace_bytes', N, Ho, Wo, O, K, KWP)
    # the weight gradient of the PACKED operator, y[n, oy, ox] = sum_kh xp[n, oy s + kh, ox s .. ox s + KWP) . w[:, kh, :]: every column of
    # the packed weight receives the correlation of dy with the input it multiplies -- also the columns beyond the kernel width, whose
    # weights the forward pass keeps at zero; channel 3 of the packed input is zero, so its gradient is
    wkt = torch.from_numpy(wk.transpose(0, 3, 1, 2).copy()).requires_grad_(True)             # (O, 4, K, KWP)
    yk = Fnn.conv2d(torch.from_numpy(want_xp.transpose(0, 3, 1, 2).copy()), wkt, None, s, 0)[:, :, :Ho, :Wo]
    assert np.array_equal(yk.detach().numpy(), y_ref)
    yk.backward(torch.from_numpy(dy))
    want_dw = dw0 + wkt.grad.numpy().transpose(0, 2, 3, 1)
    assert np.abs(want_dw).max() < cx.FP32_EXACT and not np.any(wkt.grad.numpy()[:, 3])
    for scratch in (True, False):
        ws = torch.full((max(need, 16),), 0x7f, dtype=torch.uint8, device=dev())
        dyb = Guarded(N * Ho * Wo, O, '+8' if scratch else 'dense', values=rows_nhwc(dy))
        dw = Guarded(O, K * KWP * 4, 'packed', dtype=torch.float32)
        dw.view.copy_(_f32(dw0.reshape(O, -1)))
        hip.call('sn_conv_stem_wgrad', dyb.view, xp.view, dw.view, N, Hp, Wp, Ho, Wo, O, dyb.pitch, K, KWP, s, ws if scratch else None,
                 need if scratch else 0, hip.stream())
        got = dw.result()
        bad = cx.first_mismatch(got, want_dw.reshape(O, -1))
        assert bad is None, 'sn_conv_stem_wgrad %s scratch %s: dw[%d][%d] got %r want %r' % (shape, scratch, bad[0], bad[1], float(got[bad]),
                                                                                          want_dw.reshape(O, -1)[bad])
        assert dw.untouched()
