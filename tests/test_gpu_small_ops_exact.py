"""-m gpu: the small kernels of csrc/nn_ops.hip, csrc/mask.hip and csrc/dwconv.hip -- pooling, element-wise and clip, layout
conversion, weight transposes, smooth-L1, SGD, depth <-> space, pick, sn_copy2d -- against float64 references ON THE BITS
(small_ops_util.py; DESIGN.md "Exact tests of the small kernels").  Every looped kernel runs once past its grid cap, so the second
trip of its grid-stride loop is compared element by element; every pitch of a pitched kernel differs from the others within one
call; every output lives in a guarded buffer (a sentinel around it, and in the spare lanes of its pitch, that must survive the
launch); inputs are surrounded by NaN -- or, for the kernels that compare (max-pool, ReLU, clip: fmaxf and `v > 0` swallow a NaN),
by a large finite poison."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import small_ops_util as su  # noqa: E402
from gpu_util import dev  # noqa: E402
from small_ops_util import Guarded, kinds  # noqa: E402

F16, F32 = torch.float16, torch.float32
T_OF = {0: F16, 1: F32}
NAN = float('nan')
FLAT_GUARD = 1024


def _hip():
    from sniper_amd import hip
    return hip


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev())          # (the problems' arrays are read-only)


def _in(values, kind='dense', dtype=F16, poison=NAN):
    """a (rows, C) input: `poison` in the guard rows and in the spare lanes of the pitch"""
    g = Guarded(values.shape[0], values.shape[1], kind, dtype=dtype)
    g.flat.fill_(poison)
    g.view.copy_(_dev(values))
    return g


def _out(rows, C, kind='dense', dtype=F16):
    return Guarded(rows, C, kind, dtype=dtype)


def _inout(values, kind='dense', dtype=F16):
    """an operand a launch reads AND writes: the values inside, the sentinel around them"""
    g = Guarded(values.shape[0], values.shape[1], kind, dtype=dtype)
    g.view.copy_(_dev(values))
    return g


class _Flat(Guarded):
    """Guarded for a one-dimensional operand of n elements (a row of n lanes would carry 2 x 256 guard rows of n lanes each): 1024
    guard elements on both sides, `offset` more in front.  `values` may be a whole image of the operand, spare lanes included."""

    def __init__(self, n, dtype, values=None, fill=su.SENTINEL, offset=0):
        self.rows, self.C, self.pitch, self.offset = 1, n, n, offset
        self.flat = torch.full((2 * FLAT_GUARD + offset + n,), fill, dtype=dtype, device=dev())
        self.view = self.flat[FLAT_GUARD + offset:FLAT_GUARD + offset + n]
        if values is not None:
            self.view.copy_(_dev(np.asarray(values).reshape(-1)))


def _check(buf, want, what):
    want = np.asarray(want)
    msg = su.compare(buf.result().reshape(want.shape), want, what)
    assert not msg, msg
    assert buf.untouched(), '%s: the launch wrote outside its %d x %d output (pitch %d, offset %d)' % (what, buf.rows, buf.C, buf.pitch, buf.offset)


# ------------------------------------------------------------------------------------------------------------------ sn_ew_f16
def test_ew_f16_exact():
    """modes 0 / 1 / 2, mode 2 without b, with b and with b ALIASING y; a, b, ref and y at four different pitches in every call"""
    hip = _hip()
    n = su.Counts()
    for i, case in enumerate(su.ew_cases()):
        rows, C = case
        q = su.ew_problem(case)
        small = rows * (C // 8) <= su.EW_CAP_ITEMS
        what = 'sn_ew_f16 rows %d C %d' % case
        a_fin, ref = _in(q.a, kinds(i, 0), poison=su.POISON16), _in(q.ref, kinds(i, 2), poison=su.POISON16)
        a, b = (_in(q.a, kinds(i, 0)) if small else a_fin), _in(q.b, kinds(i, 1))
        assert len({a.pitch, b.pitch, ref.pitch, su.pitch_of(C, kinds(i, 3))[0]}) == 4, case
        runs = [(0, a_fin, None, None, q.relu), (1, a, b, None, q.add), (2, a, b, ref, q.bwd_b)]
        if small:
            runs.append((2, a, None, ref, q.bwd))
        for mode, aa, bb, rr, want in runs:
            y = _out(rows, C, kinds(i, 3))
            hip.call('sn_ew_f16', aa.view, bb.view if bb else None, rr.view if rr else None, y.view, rows, C, aa.pitch,
                     bb.pitch if bb else C, rr.pitch if rr else C, y.pitch, mode, hip.stream())
            _check(y, want, '%s mode %d%s' % (what, mode, ' with b' if bb and mode == 2 else ''))
            n.add('launches')
        if small:
            y = _inout(q.b, kinds(i, 3))
            hip.call('sn_ew_f16', a.view, y.view, ref.view, y.view, rows, C, a.pitch, y.pitch, ref.pitch, y.pitch, 2, hip.stream())
            _check(y, q.bwd_b, what + ' mode 2, b aliasing y')
            n.add('launches')
            n.add('aliased')
        else:
            n.add('beyond_cap')
        n.add('cases')
    n.log('ew_f16')
    assert n['cases'] == len(su.ew_cases()) and n['beyond_cap'] == 1 and n['aliased'] == n['cases'] - 1


# ---------------------------------------------------------------------------------------------------------------- sn_clip_f16
def test_clip_f16_exact():
    """forward, and backward without `accumulate`, with one of its own and with one ALIASING y; ref exactly on lo and on hi passes
    the gradient (lo <= x <= hi, mx.sym.clip's rule).  The case past the cap is past dw_blocks' cap, read from the source."""
    hip = _hip()
    n = su.Counts()
    cases = su.clip_cases()
    for i, case in enumerate(cases):
        rows, C = case
        small = rows * (C // 8) <= su.clip_cap_items()
        for bounds in (su.CLIP_BOUNDS if small else su.CLIP_BOUNDS[:1]):
            lo, hi = bounds
            q = su.clip_problem(case, bounds)
            what = 'sn_clip_f16 rows %d C %d [%g, %g]' % (case + bounds)
            a_fin, ref = _in(q.a, kinds(i, 0), poison=su.POISON16), _in(q.ref, kinds(i, 1), poison=su.POISON16)
            y = _out(rows, C, kinds(i, 3))
            hip.call('sn_clip_f16', a_fin.view, None, None, y.view, rows, C, a_fin.pitch, C, C, y.pitch, lo, hi, 0, hip.stream())
            _check(y, q.fwd, what + ' forward')
            a = _in(q.a, kinds(i, 0)) if small else a_fin
            y = _out(rows, C, kinds(i, 3))
            hip.call('sn_clip_f16', a.view, ref.view, None, y.view, rows, C, a.pitch, ref.pitch, C, y.pitch, lo, hi, 1, hip.stream())
            _check(y, q.bwd, what + ' backward')
            n.add('launches', 2)
            n.add('on_lo_or_hi', int(((q.ref == lo) | (q.ref == hi)).sum()))
            if not small:
                n.add('beyond_cap')
                continue
            acc, y = _in(q.acc, kinds(i, 2)), _out(rows, C, kinds(i, 3))
            assert len({a.pitch, ref.pitch, acc.pitch, y.pitch}) == 4, case
            hip.call('sn_clip_f16', a.view, ref.view, acc.view, y.view, rows, C, a.pitch, ref.pitch, acc.pitch, y.pitch, lo, hi, 1, hip.stream())
            _check(y, q.bwd_acc, what + ' backward + accumulate')
            y = _inout(q.acc, kinds(i, 3))
            hip.call('sn_clip_f16', a.view, ref.view, y.view, y.view, rows, C, a.pitch, ref.pitch, y.pitch, y.pitch, lo, hi, 1, hip.stream())
            _check(y, q.bwd_acc, what + ' backward, accumulate aliasing y')
            n.add('launches', 2)
        n.add('cases')
    n.log('clip_f16')
    assert n['cases'] == len(cases) and n['beyond_cap'] == 1 and n['on_lo_or_hi'] > 0


# ------------------------------------------------------------------------------------------------------------- sn_maxpool_fwd
def _maxpool(hip, n, case):
    N, H, W, C, k, s, p = case
    q = su.pool_problem(case)
    Ho, Wo = su.pool_out(H, k, s, p), su.pool_out(W, k, s, p)
    x, y = _in(q.x.reshape(-1, C), 'dense', poison=su.POISON16), _out(N * Ho * Wo, C, 'dense')
    hip.call('sn_maxpool_fwd', x.view, y.view, N, H, W, C, k, s, p, hip.stream())
    _check(y, q.y.reshape(-1, C), 'sn_maxpool_fwd N %d H %d W %d C %d k %d s %d p %d' % case)
    n.add('launches')
    n.add('chunks', N * Ho * Wo * (C // 8))


def test_maxpool_fwd_exact():
    """against torch-CPU max_pool2d at four (k, s, p), odd / even extents, a last window cut by the border, 1 x 1 under pad 1;
    the border windows hold only negative values, the input sits in a finite poison"""
    hip = _hip()
    n = su.Counts()
    cases = [c for c in su.pool_cases() if c != su.POOL_LARGE]
    for case in cases:
        _maxpool(hip, n, case)
    n.log('maxpool_fwd')
    assert n['launches'] == len(cases) >= 30


def test_maxpool_fwd_beyond_the_grid_cap():
    hip = _hip()
    n = su.Counts()
    _maxpool(hip, n, su.POOL_LARGE)
    n.log('maxpool_fwd beyond the cap')
    assert n['chunks'] == 2099601 > su.EW_CAP_ITEMS + 256


# -------------------------------------------------------------------------------------------- sn_avgpool_global_fwd / _bwd
def test_avgpool_global_exact():
    """integer sums; forward float32(s) / float32(HW), backward float16(float32(dy) / float32(HW)): one correctly rounded division
    (hipcc's default for `/` on floats), so the comparison is on the bits"""
    hip = _hip()
    n = su.Counts()
    for i, case in enumerate(su.avg_cases()):
        N, HW, C = case
        q = su.avg_problem(case)
        what = 'N %d HW %d C %d' % case
        x, y = _in(q.x.reshape(-1, C), 'packed'), _Flat(N * C, F32, offset=(0, 1, 8, 3)[i % 4])
        hip.call('sn_avgpool_global_fwd', x.view, y.view, N, HW, C, hip.stream())
        _check(y, q.y.reshape(-1), 'sn_avgpool_global_fwd ' + what)
        dy, dx = _Flat(N * C, F32, q.dy, fill=NAN, offset=(1, 0, 3, 8)[i % 4]), _out(N * HW, C, 'packed')
        hip.call('sn_avgpool_global_bwd', dy.view, dx.view, N, HW, C, hip.stream())
        _check(dx, q.dx.reshape(-1, C), 'sn_avgpool_global_bwd ' + what)
        n.add('launches', 2)
        n.add('cases')
    n.log('avgpool_global')
    assert n['cases'] == len(su.avg_cases()) == 18


# -------------------------------------------------------------------------------------------------------- sn_transpose_batched
def _transpose(hip, n, case, pair, exact):
    batch = su.tr_batch(case, pair)
    _, r, c, in_ld, out_ld, ibs, obs = case
    ti, to = pair
    vals = su.tr_values(case, batch, exact)
    src, dst = su.tr_images(case, batch, vals, NAN, su.SENTINEL, su.NP_OF[to])
    x, y = _Flat(src.size, T_OF[ti], src, fill=NAN), _Flat(dst.size, T_OF[to])
    hip.call('sn_transpose_batched', x.view, y.view, batch, r, c, ibs, obs, in_ld, out_ld, ti, to, hip.stream())
    _check(y, dst, 'sn_transpose_batched batch %d rows %d cols %d in_ld %d out_ld %d strides %d / %d dtypes %d -> %d%s'
           % (batch, r, c, in_ld, out_ld, ibs, obs, ti, to, '' if exact else ' (rounding)'))
    n.add('launches')
    n.add('batch_%d' % batch)


@pytest.mark.parametrize('pair', su.TR_DTYPES, ids=lambda p: '%s->%s' % tuple('f16 f32'.split()[d] for d in p))
def test_transpose_batched_exact(pair):
    """rows and cols on both sides of the 32 x 32 tile, in_ld > cols, out_ld > rows, slack between the batches; the expected image
    of the WHOLE output buffer -- the sentinel in every spare lane -- is compared.  fp32 -> fp16 runs again on values that are no
    fp16 values (round to nearest even); fp32 -> fp32 carries such values unchanged."""
    hip = _hip()
    n = su.Counts()
    for case in su.tr_cases():
        if pair != (1, 1):
            _transpose(hip, n, case, pair, True)
        if pair[0] == 1:
            _transpose(hip, n, case, pair, False)
    n.log('transpose_batched %d -> %d' % pair)
    assert n['launches'] == len(su.tr_cases()) * (2 if pair == (1, 0) else 1) and n['batch_1'] and n['batch_3']


# ------------------------------------------------------------------------- sn_weight_transpose / sn_weight_transpose_batched
def test_weight_transpose_exact():
    """single launches (the last shape past the grid cap) and one batched table whose descriptor search lands on the first, the
    middle and the last entry; columns O..Opad-1 are zero, the destination is guarded"""
    hip = _hip()
    n = su.Counts()
    for shape in su.WT_SHAPES:
        O, T, I, Opad = shape
        q = su.wt_problem(shape)
        src, dst = _Flat(q.w.size, F32, q.w, fill=NAN), _Flat(q.wt.size, F16)
        hip.call('sn_weight_transpose', src.view, dst.view, O, T, I, Opad, hip.stream())
        _check(dst, q.wt.reshape(-1), 'sn_weight_transpose O %d T %d I %d Opad %d' % shape)
        n.add('launches')
        n.add('beyond_cap', int(q.wt.size > su.EW_CAP_ITEMS + 256))
    shapes = [su.WT_SHAPES[k] for k in su.WT_TABLE]
    qs = [su.wt_problem(s) for s in shapes]
    srcs = [_Flat(q.w.size, F32, q.w, fill=NAN, offset=(0, 4, 12, 0, 8)[k]) for k, q in enumerate(qs)]
    dsts = [_Flat(q.wt.size, F16) for q in qs]
    rec, tiles = su.wt_table(shapes, [s.view.data_ptr() for s in srcs], [d.view.data_ptr() for d in dsts])
    desc = _dev(rec.view(np.uint8).copy())
    hip.call('sn_weight_transpose_batched', desc, len(shapes), tiles, hip.stream())
    for k, (shape, q, d) in enumerate(zip(shapes, qs, dsts)):
        _check(d, q.wt.reshape(-1), 'sn_weight_transpose_batched entry %d of %d: O %d T %d I %d Opad %d' % ((k, len(shapes)) + shape))
    n.add('launches')
    n['table'], n['tiles'] = len(shapes), tiles
    n.log('weight_transpose')
    assert n['beyond_cap'] == 1 and n['table'] >= 3


# ---------------------------------------------------------------------------------------------------------- sn_smooth_l1_loss
@pytest.mark.parametrize('sigma', su.SL1_SIGMA)
def test_smooth_l1_exact(sigma):
    """sigma 1 and 3 (the RPN's); with `loss` null, with `dpred` null and with both; n on both sides of a block and past the cap"""
    hip = _hip()
    n = su.Counts()
    for i, case in enumerate(c for c in su.sl1_cases() if c[1] == sigma):
        cnt = case[0]
        q = su.sl1_problem(case)
        pred, target, w = [_Flat(cnt, F32, v, fill=NAN, offset=(k + i) % 4 * 4) for k, v in enumerate((q.pred, q.target, q.w))]
        for form in ('both', 'dpred only', 'loss only'):
            loss = _Flat(cnt, F32, offset=i % 3) if form != 'dpred only' else None
            dp = _Flat(cnt, F32, offset=(i + 1) % 3) if form != 'loss only' else None
            hip.call('sn_smooth_l1_loss', pred.view, target.view, w.view, loss.view if loss else None, dp.view if dp else None, cnt,
                     float(sigma), su.SL1_GRAD_SCALE, hip.stream())
            what = 'sn_smooth_l1_loss n %d sigma %g (%s)' % (cnt, sigma, form)
            if loss:
                _check(loss, q.loss, what + ' loss')
            if dp:
                _check(dp, q.dpred, what + ' dpred')
            n.add('launches')
        n.add('cases')
        n.add('quadratic', int(q.quadratic.sum()))
        n.add('linear', int((~q.quadratic).sum()))
    n.log('smooth_l1 sigma %g' % sigma)
    assert n['cases'] == len(su.SL1_N) and n['launches'] == 3 * n['cases'] and n['quadratic'] > 1000 and n['linear'] > 1000


# --------------------------------------------------------------------- sn_sgd_mom_update, _dev, _guarded_dev
def _state(coef=1.0, skip=0.0):
    """the guard's device state: [1] the clipping coefficient, [2] the skip flag"""
    return torch.tensor([1.0, coef, skip, 0.0, 0.0, skip, skip, 1.0], dtype=torch.float64, device=dev())


def _sgd(hip, n, case, kernel, guard=None):
    """one update of the slice [off, off + n) of four arrays that each start at their own offset; all four are compared WHOLE: the
    elements outside the slice keep their bits.  guard = (coef, clip, skip)"""
    cnt, offs, mode = case
    q = su.sgd_problem(cnt)
    o16 = su.w16_offset(offs[0], mode)
    frs = np.random.RandomState(su.case_seed(case))
    imgs = [su.sgd_image(v, o, frs, -64, 64, 0.125, np.float32) for v, o in zip((q.w, q.g, q.m), offs)]
    h_img = su.sgd_image(q.h, o16, frs, -64, 64, 1.0, np.float16) if o16 is not None else None
    w, g, m = [_dev(a) for a in imgs]
    h = _dev(h_img) if h_img is not None else None
    sl = [t[su.SGD_PAD + o:] for t, o in zip((w, g, m), offs)] + [h[su.SGD_PAD + o16:] if h is not None else None]
    assert all(t.data_ptr() % 16 == 0 for t in (w, g, m)) and (h is None or h.data_ptr() % 16 == 0)
    tag = ''
    if kernel == 'sn_sgd_mom_update':
        hip.call(kernel, sl[0], sl[1], sl[2], sl[3], cnt, *(su.SGD_HYPER + (hip.stream(),)))
    else:
        hyper = torch.tensor(su.SGD_DEV_HYPER, dtype=F32, device=dev())
        if guard is None:
            hip.call(kernel, sl[0], sl[1], sl[2], sl[3], cnt, hyper, su.SGD_MULTS[0], su.SGD_MULTS[1], hip.stream())
        else:
            coef, clip, skip = guard
            hip.call(kernel, sl[0], sl[1], sl[2], sl[3], cnt, hyper, su.SGD_MULTS[0], su.SGD_MULTS[1], float(clip), _state(coef, skip),
                     hip.stream())
            tag = '_guard' if (coef, clip) != (1.0, 0.0) else ''
    skip = guard is not None and guard[2]
    what = '%s n %d offsets %r w16 %s%s' % (kernel, cnt, offs, mode, (' guard %r' % (guard,)) if guard else '')
    wants = []
    for img, o, name in zip(imgs + [h_img], offs + (o16,), ('w1', None, 'm1', 'h1')):
        if img is None:
            wants.append(None)
            continue
        want = img.astype(np.float64)
        if name and not skip:
            want[su.SGD_PAD + o:su.SGD_PAD + o + cnt] = getattr(q, name + tag)
        wants.append(want)
    msgs = [su.compare(t.cpu().numpy(), want, '%s: %s' % (what, name)) for t, want, name in zip((w, g, m, h), wants, ('w32', 'grad', 'mom', 'w16'))
            if t is not None]
    assert not any(msgs), '\n'.join(x for x in msgs if x)
    n.add('launches')
    n.add('vector path' if su.sgd_vector_path(offs, mode) else 'fallback')


def _sgd_small_cases():
    return [c for c in su.sgd_cases() if c[0] != su.SGD_LARGE_N]


def test_sgd_dev_exact():
    """every start-offset combination: all equal (head / four-wide body / tail) and one array differing (the scalar fallback);
    without the fp16 copy, with it 8- but not 16-byte aligned behind the head, and misaligned"""
    hip = _hip()
    n = su.Counts()
    for case in _sgd_small_cases():
        _sgd(hip, n, case, 'sn_sgd_mom_update_dev')
    n.log('sgd_mom_update_dev')
    assert n['launches'] == len(_sgd_small_cases()) and n['vector path'] >= 4 * 3 * len(su.SGD_N) and n['fallback'] >= 36 * len(su.SGD_N)


def test_sgd_guarded_dev_exact():
    """the guarded statement (coefficient 0.5, clip 0.25) over the same offsets; with nothing to apply the plain statement's bits;
    with the skip flag set nothing is written"""
    hip = _hip()
    n = su.Counts()
    for case in _sgd_small_cases():
        _sgd(hip, n, case, 'sn_sgd_mom_update_guarded_dev', su.SGD_GUARD + (0.0,))
        if case[1][0] == case[1][1] == case[1][2] or case[0] == 1027:
            _sgd(hip, n, case, 'sn_sgd_mom_update_guarded_dev', (1.0, 0.0, 0.0))
            _sgd(hip, n, case, 'sn_sgd_mom_update_guarded_dev', su.SGD_GUARD + (1.0,))
            n.add('skipped')
    n.log('sgd_mom_update_guarded_dev')
    assert n['launches'] == len(_sgd_small_cases()) + 2 * n['skipped'] and n['skipped'] >= 16 * len(su.SGD_N)


def test_sgd_plain_exact():
    """the host-hyper-parameter form (one scalar kernel, no split) over the same offsets: the same bits"""
    hip = _hip()
    n = su.Counts()
    for case in _sgd_small_cases():
        _sgd(hip, n, case, 'sn_sgd_mom_update')
    n.log('sgd_mom_update')
    assert n['launches'] == len(_sgd_small_cases())


def test_sgd_beyond_the_grid_cap():
    """n = 4 * EW_CAP_ITEMS + 4 * 257 + 3 at offset 3: a head of 1, a body of EW_CAP_ITEMS + 257 float4, a tail of 2"""
    hip = _hip()
    n = su.Counts()
    case = su.sgd_cases()[-1]
    assert case[0] == su.SGD_LARGE_N and (case[0] - su.sgd_head(case[1][0])) // 4 > su.EW_CAP_ITEMS + 256
    _sgd(hip, n, case, 'sn_sgd_mom_update')
    _sgd(hip, n, case, 'sn_sgd_mom_update_dev')
    _sgd(hip, n, case, 'sn_sgd_mom_update_guarded_dev', su.SGD_GUARD + (0.0,))
    _sgd(hip, n, case, 'sn_sgd_mom_update_guarded_dev', su.SGD_GUARD + (1.0,))
    n.log('sgd beyond the cap')
    assert n['launches'] == 4


# ------------------------------------------------------------------------------- sn_depth_to_space2 / sn_space_to_depth2
@pytest.mark.parametrize('case', su.ds_cases(), ids=lambda c: 'x'.join(map(str, c)))
def test_depth_space_exact(case):
    """both directions, relu on and off, and the round trip of the device's own output; the last case is past the 16384-block cap"""
    hip = _hip()
    n = su.Counts()
    N, H, W, C = case
    q = su.ds_problem(case)
    what = 'N %d H %d W %d C %d' % case
    deep = _in(q.deep.reshape(-1, 4 * C), 'dense', poison=su.POISON16)
    small = su.ds_items(case) <= su.DS_CAP_ITEMS
    for relu in ((0, 1) if small else (1,)):
        space = _out(N * 2 * H * 2 * W, C, 'dense')
        hip.call('sn_depth_to_space2', deep.view, space.view, N, H, W, C, relu, hip.stream())
        _check(space, (q.space_relu if relu else q.space).reshape(-1, C), 'sn_depth_to_space2 %s relu %d' % (what, relu))
        n.add('launches')
    src = _in(q.space.reshape(-1, C), 'dense')
    back = _out(N * H * W, 4 * C, 'dense')
    hip.call('sn_space_to_depth2', src.view, back.view, N, H, W, C, hip.stream())
    _check(back, q.deep.reshape(-1, 4 * C), 'sn_space_to_depth2 ' + what)
    n.add('launches')
    if small:
        space, back = _out(N * 2 * H * 2 * W, C, 'dense'), _out(N * H * W, 4 * C, 'dense')
        hip.call('sn_depth_to_space2', deep.view, space.view, N, H, W, C, 0, hip.stream())
        hip.call('sn_space_to_depth2', space.view, back.view, N, H, W, C, hip.stream())
        assert torch.equal(back.view.view(torch.int16), deep.view.view(torch.int16)), what + ': the round trip is not the identity'
        n.add('launches', 2)
    n['items'] = su.ds_items(case)
    n.log('depth_space %s' % what)


# ------------------------------------------------------------------------------------------------- sn_pick_fwd / sn_pick_bwd
def test_pick_exact():
    """indices below 0 and at or above C clip; the forward also at C = 5; the backward overwrites or accumulates, the picked channel
    in the first, a middle and the last 8-channel chunk; N * HW = 255, 256, 257"""
    hip = _hip()
    n = su.Counts()
    for i, case in enumerate(su.pick_cases(True)):
        N, HW, C = case
        q = su.pick_problem(case)
        what = 'N %d HW %d C %d' % case
        x, idx = _in(q.x.reshape(-1, C), 'packed' if C % 8 else 'dense'), _Flat(N, F32, q.index, fill=NAN, offset=i % 4)
        y = _Flat(N * HW, F16, offset=(0, 8, 1)[i % 3])
        hip.call('sn_pick_fwd', x.view, idx.view, y.view, N, HW, C, hip.stream())
        _check(y, q.y.reshape(-1), 'sn_pick_fwd ' + what)
        n.add('launches')
        if case not in su.pick_cases(False):
            continue
        dy = _Flat(N * HW, F16, q.dy, fill=NAN, offset=(1, 0, 8)[i % 3])
        dx = _out(N * HW, C, 'dense')
        hip.call('sn_pick_bwd', dy.view, idx.view, dx.view, N, HW, C, 0, hip.stream())
        _check(dx, q.dx.reshape(-1, C), 'sn_pick_bwd ' + what)
        dx = _inout(q.dx0.reshape(-1, C), 'dense')
        hip.call('sn_pick_bwd', dy.view, idx.view, dx.view, N, HW, C, 1, hip.stream())
        _check(dx, q.dx_acc.reshape(-1, C), 'sn_pick_bwd accumulate ' + what)
        n.add('launches', 2)
        n.add('bwd_cases')
    n.log('pick')
    assert n['launches'] == len(su.pick_cases(True)) + 2 * len(su.pick_cases(False)) and n['bwd_cases'] == 6


# ------------------------------------------------------------------------------------------------------------------ sn_copy2d
@pytest.mark.parametrize('case', (su.COPY_SCALAR, su.COPY_VEC8), ids=('scalar', 'vec8'))
def test_copy2d_beyond_the_grid_cap(case):
    """what test_copy2d_vectorised_and_scalar_paths lacks: the element-wise kernel and the 16-byte kernel past the grid cap"""
    hip = _hip()
    n = su.Counts()
    rows, cols, in_ld, out_ld, ti, to = case
    q = su.copy_problem(case)
    src = np.full((rows, in_ld), np.nan, np.float32)
    src[:, :cols] = q.x
    dst = np.full((rows, out_ld), su.SENTINEL, np.float32)
    dst[:, :cols] = q.x
    src, dst = src.reshape(-1)[:(rows - 1) * in_ld + cols], dst.reshape(-1)[:(rows - 1) * out_ld + cols]
    x, y = _Flat(src.size, T_OF[ti], src, fill=NAN), _Flat(dst.size, T_OF[to])
    hip.call('sn_copy2d', x.view, y.view, rows, cols, in_ld, out_ld, ti, to, hip.stream())
    _check(y, dst, 'sn_copy2d rows %d cols %d in_ld %d out_ld %d dtypes %d -> %d' % case)
    n.add('launches')
    n['items'] = su.copy_items(case)
    n.log('copy2d %s' % ('scalar' if cols % 8 else 'vec8'))
    assert n['items'] > su.EW_CAP_ITEMS + 256
