"""CPU: the case lists, operands and references of the small kernels' exact tests (small_ops_util.py; the launches are in
test_gpu_small_ops_exact.py).  Four things, none of which needs a device: every problem meets the exactness conditions its zero
tolerance rests on; every case list reaches the edges it is there for (one case per looped kernel past its grid cap among them);
the caps this module assumes are the literals in the sources; and the comparison is sensitive -- the expected arrays are perturbed
the way a particular kernel bug would perturb the output, and the comparator must name the right element.  No mutated kernel is
ever built or run."""
import itertools

import numpy as np

import small_ops_util as su
from small_ops_util import F16, F32, F64, first_mismatch


# ---------------------------------------------------------------------------------------------------------------- exactness
def _problems():
    for c in su.ew_cases():
        yield su.ew_problem(c)
    for c in su.clip_cases():
        small = c[0] * c[1] // 8 <= su.clip_cap_items()
        for b in (su.CLIP_BOUNDS if small else su.CLIP_BOUNDS[:1]):
            yield su.clip_problem(c, b)
    for c in su.pool_cases():
        yield su.pool_problem(c)
    for c in su.avg_cases():
        yield su.avg_problem(c)
    for s in su.WT_SHAPES:
        yield su.wt_problem(s)
    for c in su.sl1_cases():
        yield su.sl1_problem(c)
    for n in su.SGD_N + (su.SGD_LARGE_N,):
        yield su.sgd_problem(n)
    for c in su.ds_cases():
        yield su.ds_problem(c)
    for c in su.pick_cases(True):
        yield su.pick_problem(c)
    for c in (su.COPY_SCALAR, su.COPY_VEC8):
        yield su.copy_problem(c)


def test_every_problem_meets_its_exactness_conditions():
    count = 0
    for q in _problems():
        su.check_exact(q)
        count += 1
    assert count >= 100
    for cached in (su.ew_problem, su.clip_problem, su.pool_problem, su.sl1_problem, su.sgd_problem, su.ds_problem, su.copy_problem):
        cached.cache_clear()               # (the problems past the caps are 30 -- 130 MB per array)


def test_the_check_refuses_inexact_operands():
    q = su.Prob('x')
    q.put('a', np.array([0.1]), F32)
    try:
        su.check_exact(q)
    except AssertionError:
        pass
    else:
        raise AssertionError('0.1 passed as an fp32 value')
    assert su.survives(np.array([2048.0, -0.125]), F16) and not su.survives(np.array([2049.0]), F16)
    assert not su.survives(np.array([70000.0]), F16) and not su.survives(np.array([np.nan]), F32)


def test_single_roundings_are_applied_to_exact_values():
    # fp32 -> fp16 stores of the SGD copy: w' needs up to 13 bits, the store rounds some of them
    q = su.sgd_problem(1027)
    assert set(q.rounded) == {'h1', 'h1_guard'}
    assert (q.h1.astype(F64) != q.w1).any() and np.abs(q.h1.astype(F64) - q.w1).max() <= 2.0 ** -9
    assert (q.w1 != q.w1_guard).any()                                     # the clip and the coefficient change the update
    # the average pool: both operands of the one division are exact, the quotient is not (HW = 49), the reference is numpy's
    # correctly rounded fp32 division
    q = su.avg_problem((3, 49, 81))
    assert su.survives(q.s, F32) and su.survives(q.dy, F32) and su.survives(q.hw, F32)
    assert q.y.dtype == F32 and np.array_equal(q.y, (q.s / 49.0).astype(F32)) and not su.survives(q.s / 49.0, F32)
    assert q.dx.dtype == F16 and np.array_equal(q.dx[:, 0, :], (q.dy.astype(F32) / F32(49)).astype(F16))
    assert all(su.survives(su.avg_problem(c).s / c[1], F32) for c in su.avg_cases() if c[1] in (1, 64))
    # smooth-L1 under sigma = 3: th = float32(1 / 9) is no dyadic number, |d| - th / 2 is exact in float64 and rounded once
    q = su.sl1_problem((257, 3.0))
    assert q.th == float(F32(1.0) / F32(9.0)) and su.survives(q.half_th, F32)
    lin = ~q.quadratic
    assert lin.any() and q.quadratic.any()
    big = np.abs(q.d) + 0.0
    assert np.array_equal((q.lin_exact + 0.5 * q.th)[lin], big[lin])                      # the float64 difference lost nothing
    assert not su.survives(q.lin_exact[lin], F32) and su.survives(q.lin[lin], F32)
    q1 = su.sl1_problem((257, 1.0))
    assert q1.th == 1.0 and su.survives(q1.lin_exact, F32)
    # fp32 -> fp16 of the transposes' second run: thirds are fp32 values and no fp16 values
    v = su.tr_values(su.tr_cases()[7], 3, False)
    assert su.survives(v, F32) and not su.survives(v, F16) and su.survives(su.tr_values(su.tr_cases()[7], 3, True), F16)


# -------------------------------------------------------------------------------------------------------------------- reach
def test_caps_are_the_sources_literals():
    caps = su.source_caps()
    assert caps['ew'] == su.EW_CAP_ITEMS == 8192 * 256
    assert caps['ds'] == su.DS_CAP_ITEMS == 16384 * 256
    assert caps['dw'] == su.clip_cap_items() and caps['dw'] % 256 == 0 and caps['dw'] >= 256
    # the launchers under test do size their grids by these functions
    nn, dw = su._src('nn_ops.hip'), su._src('dwconv.hip')
    for kernel in ('ew_f16_kernel', 'maxpool_kernel', 'smooth_l1_kernel', 'sgd_kernel', 'sgd_dev_kernel', 'sgd_dev_vec4_kernel',
                   'sgd_guard_kernel', 'sgd_guard_vec4_kernel', 'weight_oti_to_ito_kernel', '(copy2d_vec8_kernel<TI, TO>)',
                   '(copy2d_kernel<TI, TO>)'):
        assert 'hipLaunchKernelGGL(%s, dim3(ew_blocks(' % kernel in nn, kernel
    assert 'hipLaunchKernelGGL(clip_f16_kernel, dim3(dw_blocks(' in dw


def test_every_looped_kernel_has_a_case_past_its_cap():
    past = su.EW_CAP_ITEMS + 256
    assert sum(r * (c // 8) > past for r, c in su.ew_cases()) == 1 and su.EW_LARGE == (su.EW_CAP_ITEMS + 257, 8)
    assert sum(r * (c // 8) > su.clip_cap_items() + 256 for r, c in su.clip_cases()) == 1
    N, H, W, C, k, s, p = su.POOL_LARGE
    assert su.pool_cases()[-1] == su.POOL_LARGE and N * su.pool_out(H, k, s, p) * su.pool_out(W, k, s, p) * (C // 8) == 2099601 > past
    assert max(np.prod(s[1:]) for s in su.WT_SHAPES) > past and su.WT_SHAPES[-1] == (512, 9, 512, 512)
    assert max(su.SL1_N) == su.EW_CAP_ITEMS + 257 and all((max(su.SL1_N), s) in su.sl1_cases() for s in (1.0, 3.0))
    n, offs, mode = su.sgd_cases()[-1]
    head = su.sgd_head(offs[0])
    assert n == 4 * su.EW_CAP_ITEMS + 4 * 257 + 3 and su.sgd_vector_path(offs, mode) and mode != 'none'
    assert head > 0 and (n - head) // 4 > past and (n - head) % 4 > 0 and n > past          # head, body past the cap, tail
    assert su.ds_items(su.DS_LARGE) > su.DS_CAP_ITEMS + 256 and su.ds_cases()[-1] == (1, 1025, 1025, 8)
    assert all(su.ds_items(c) <= su.DS_CAP_ITEMS for c in su.DS_CASES)
    assert su.copy_items(su.COPY_SCALAR) > past and su.COPY_SCALAR[1] % 8 != 0
    rows, cols, in_ld, out_ld = su.COPY_VEC8[:4]
    assert su.copy_items(su.COPY_VEC8) > past and cols % 8 == 0 and in_ld % 8 == 0 and out_ld % 8 == 0 and in_ld != out_ld


def test_elementwise_cases_reach_their_edges():
    assert {c for _, c in su.ew_cases()} == {8, 24, 72} and {r for r, _ in su.ew_cases()} >= {1, 7, 257}
    assert su.clip_cases()[:-1] == su.ew_cases()[:-1]
    for i, (rows, C) in enumerate(su.ew_cases()):
        pitches = [su.pitch_of(C, su.kinds(i, k))[0] for k in range(4)]
        assert len(set(pitches)) == 4 and min(pitches) >= C, ((rows, C), pitches)           # all four differ within one call
        q = su.ew_problem((rows, C))
        if rows * C >= 56:
            assert (q.ref == 0).any() and (q.ref > 0).any() and (q.ref < 0).any()
            assert (q.bwd != q.a).any() and (q.relu != q.a).any()
    for case in su.clip_cases()[:-1]:
        for (lo, hi) in su.CLIP_BOUNDS:
            q = su.clip_problem(case, (lo, hi))
            if case[0] * case[1] >= 56:
                on = (q.ref == lo) | (q.ref == hi)
                assert on.any() and (q.bwd[on] == q.a[on]).all() and (q.a[on] != 0).any()     # the edges pass the gradient
                assert (q.ref < lo).any() and (q.ref > hi).any() and (q.fwd != q.a).any()
    assert su.POISON16 > 2048 and su.survives(np.array([su.POISON16]), F16)


def test_pool_cases_reach_their_edges():
    cases = su.pool_cases()
    assert {c[4:] for c in cases} == set(su.POOL_GEOMS) == {(3, 2, 1), (2, 2, 0), (3, 1, 1), (3, 2, 0)}
    assert {c[3] for c in cases} == {8, 24}
    assert any(c[1:3] == (1, 1) and c[6] == 1 for c in cases)                              # 1 x 1 under pad 1
    assert any(c[1] % 2 != c[2] % 2 for c in cases)                                        # odd / even mixes
    # a last window cut by the border: its last tap lies past the input
    assert any((su.pool_out(c[1], *c[4:]) - 1) * c[5] - c[6] + c[4] > c[1] for c in cases)
    for case in cases[:-1]:
        N, H, W, C, k, s, p = case
        q = su.pool_problem(case)
        assert q.y.shape == (N, su.pool_out(H, k, s, p), su.pool_out(W, k, s, p), C)
        if p > 0:          # every border window is negative: a padding tap that contributed 0 would have won it
            assert (q.y[:, 0] < 0).all() and (q.y[:, :, 0] < 0).all() and (q.x[:, 0] < 0).all()
    assert (su.pool_problem((2, 8, 5, 8, 3, 1, 1)).y > 0).any()                            # ... and the interior is not


def test_avgpool_and_pick_cases_reach_their_edges():
    assert {c[2] for c in su.avg_cases()} == {1, 5, 81} and {c[1] for c in su.avg_cases()} == {1, 49, 64}
    for C in (1, 5, 81):
        nc = {c[0] * c[2] for c in su.avg_cases() if c[2] == C}
        assert min(nc) < 256 < max(nc), nc
    assert sorted({N * HW for N, HW, _ in su.pick_cases(True)}) == [255, 256, 257]
    assert {c[2] for c in su.pick_cases(True)} == {5, 8, 24} and {c[2] for c in su.pick_cases(False)} == {8, 24}
    for case in su.pick_cases(True):
        N, HW, C = case
        q = su.pick_problem(case)
        assert (q.index < 0).any() and (q.index >= C).any() and q.clipped.min() == 0 and q.clipped.max() == C - 1
        if C == 24:
            assert {int(c) // 8 for c in q.clipped} == {0, 1, 2}                            # first, middle and last chunk
        assert (q.dx_acc != q.dx0).any() and (q.dx != 0).sum() <= N * HW


def test_transpose_cases_reach_their_edges():
    cases = su.tr_cases()
    assert {(c[1], c[2]) for c in cases} == set(itertools.product((1, 31, 32, 33, 65), (1, 3, 32, 40, 81)))
    assert any(c[3] > c[2] for c in cases) and any(c[4] > c[1] for c in cases) and any(c[3] > c[2] and c[4] > c[1] for c in cases)
    assert all(c[5] > c[1] * c[3] and c[6] > c[2] * c[4] for c in cases)                   # the batch strides have slack
    for pair in su.TR_DTYPES:
        assert {su.tr_batch(c, pair) for c in cases} == {1, 3}
    for r in su.TR_ROWS:
        assert {su.tr_batch(c, (0, 0)) for c in cases if c[1] == r} | {su.tr_batch(c, (0, 1)) for c in cases if c[1] == r} == {1, 3}
    shapes = [su.WT_SHAPES[k] for k in su.WT_TABLE]
    rec, tiles = su.wt_table(shapes, [0] * len(shapes), [0] * len(shapes))
    assert rec.dtype.itemsize == 48 and len(shapes) >= 3 and tiles == int(rec['tile0'][-1]) + 1
    assert set(shapes) == set(su.WT_SHAPES) and shapes[0] == shapes[-1] == (1, 1, 1, 8) and max(shapes) in shapes[1:-1]
    assert any(o < op for o, _, _, op in su.WT_SHAPES) and any(o == op for o, _, _, op in su.WT_SHAPES)


def test_loss_and_update_cases_reach_their_edges():
    for case in su.sl1_cases():
        q = su.sl1_problem(case)
        if case[0] >= 255:
            assert (q.d == 0).any() and (q.d > 0).any() and (q.d < 0).any() and set(q.w) == set(su.SL1_W) == {0.0, 0.5, 1.0, 2.0}
            assert q.quadratic.sum() > 50 and (~q.quadratic).sum() > 50
            assert q.quadratic[1] and not q.quadratic[2] if case[1] == 3.0 else True       # 7/64 < 1/9 < 8/64
    offs = su.sgd_offsets()
    assert len(offs) == len(set(offs)) == 40 and sum(a == b == c for a, b, c in offs) == 4
    assert all(len({a, b, c}) <= 2 for a, b, c in offs)
    cases = su.sgd_cases()
    assert {c[0] for c in cases} == {1, 2, 3, 4, 5, 1027, su.SGD_LARGE_N} and {(c[0], c[1]) for c in cases[:-1]} == set(itertools.product(su.SGD_N, offs))
    for ow in range(4):
        head = su.sgd_head(ow)
        assert (su.SGD_PAD + ow + head) % 4 == 0
        o16 = su.w16_offset(ow, 'half8')
        assert (o16 + head) % 4 == 0 and (o16 + head) % 8 == 4                              # 8- but not 16-byte aligned
        assert (su.w16_offset(ow, 'odd') + head) % 4 != 0
        assert su.sgd_vector_path((ow,) * 3, 'none') and su.sgd_vector_path((ow,) * 3, 'half8') and not su.sgd_vector_path((ow,) * 3, 'odd')
        for n in su.SGD_N:
            assert {c[2] for c in cases if c[0] == n and c[1] == (ow,) * 3} == set(su.W16_MODES)
    assert not any(su.sgd_vector_path(o, 'same') for o in offs if len(set(o)) == 2)
    assert {c[2] for c in cases if len(set(c[1])) == 2} == set(su.W16_MODES)
    assert su.SGD_PAD % 8 == 0 and su.SGD_HYPER == (2.0 ** -4, 2.0 ** -3, 0.5, 0.25) and su.SGD_GUARD == (0.5, 0.25)
    assert tuple(h * m for h, m in zip(su.SGD_DEV_HYPER[:2], su.SGD_MULTS)) == su.SGD_HYPER[:2] and su.SGD_DEV_HYPER[2:] == su.SGD_HYPER[2:]
    q = su.sgd_problem(1027)
    assert (np.abs(q.u) > su.SGD_GUARD[1]).any() and (np.abs(q.u_guard) == su.SGD_GUARD[1]).any()
    assert {(c[1], c[2], c[3] // 8) for c in su.ds_cases()} >= {(3, 5, 1), (5, 3, 3)} and all(c[1] % 2 and c[2] % 2 for c in su.ds_cases())


# -------------------------------------------------------------------------------------------------- comparator sensitivity
def test_b_read_at_refs_pitch_is_a_mismatch_in_row_1():
    i, case = 4, su.ew_cases()[4]
    rows, C = case
    assert rows > 1
    q = su.ew_problem(case)
    body, ps_b, off_b = su.as_buffer(q.b, C, su.kinds(i, 1), np.nan)
    ps_ref = su.pitch_of(C, su.kinds(i, 2))[0]
    assert ps_b != ps_ref
    assert np.array_equal(su.read_at_pitch(body, off_b, C, rows, ps_b), q.b)
    got = (q.bwd + su.read_at_pitch(body, off_b, C, rows, ps_ref)).astype(F16)
    assert first_mismatch(q.bwd_b.astype(F16), q.bwd_b) is None
    bad = first_mismatch(got, q.bwd_b)
    assert bad is not None and bad[0] == 1, bad                     # row 0 starts at the same address under either pitch
    assert su.compare(got, q.bwd_b, 'x').startswith('x: ')


def test_a_skipped_last_chunk_is_a_mismatch_at_its_first_channel():
    for case in ((7, 24), (257, 72)):
        q = su.ew_problem(case)
        for row in (0, case[0] - 1):
            got = q.add.astype(F16)
            got[row, case[1] - 8:] = su.SENTINEL
            assert first_mismatch(got, q.add) == (row, case[1] - 8)


def test_items_past_the_grid_cap_left_untouched_are_a_mismatch_at_the_cap():
    q = su.ew_problem(su.EW_LARGE)
    got = q.relu.astype(F16)
    got.reshape(-1, 8)[su.EW_CAP_ITEMS:] = su.SENTINEL               # one item = one 8-channel chunk
    assert first_mismatch(got, q.relu) == (su.EW_CAP_ITEMS, 0)
    q = su.sl1_problem((su.EW_CAP_ITEMS + 257, 3.0))
    got = q.loss.astype(F32)
    got[su.EW_CAP_ITEMS:] = su.SENTINEL
    assert first_mismatch(got, q.loss) == (su.EW_CAP_ITEMS,)
    q = su.ds_problem(su.DS_LARGE)
    got = q.space.astype(F16).reshape(-1, 8)
    got[su.DS_CAP_ITEMS:] = su.SENTINEL
    assert first_mismatch(got, q.space.reshape(-1, 8)) == (su.DS_CAP_ITEMS, 0)


def test_a_padding_tap_that_contributes_zero_is_a_mismatch_in_the_first_window():
    for case in su.pool_cases()[:-1]:
        N, H, W, C, k, s, p = case
        q = su.pool_problem(case)
        got = su.pool_ref(q.x, k, s, p, pad_value=0.0).astype(F16)
        if p == 0:
            assert first_mismatch(got, q.y) is None
        else:
            assert first_mismatch(got, q.y) == (0, 0, 0, 0), case
    # ... and a stray read of the finite poison wins its window
    case = (2, 7, 6, 8, 3, 2, 1)
    q = su.pool_problem(case)
    assert first_mismatch(su.pool_ref(q.x, 3, 2, 1, pad_value=su.POISON16).astype(F16), q.y) == (0, 0, 0, 0)


def test_one_element_of_the_sgd_tail_not_updated_is_a_mismatch_there():
    n, off = 1027, 3
    q = su.sgd_problem(n)
    head = su.sgd_head(off)
    tail = (n - head) % 4
    assert head == 1 and tail == 2
    rs = np.random.RandomState(0)
    for name, new in (('w', q.w1), ('m', q.m1)):
        img = su.sgd_image(getattr(q, name), off, rs, -64, 64, 0.125, F32)
        want = img.astype(F64)
        want[su.SGD_PAD + off:su.SGD_PAD + off + n] = new
        assert first_mismatch(want.astype(F32), want) is None
        got = want.astype(F32)
        last = su.SGD_PAD + off + n - 1
        got[last] = img[last]
        assert img[last] != want[last] or name == 'w'
        if img[last] != want[last]:
            assert first_mismatch(got, want) == (last,)
    # an element outside the slice that was written is one too
    img = su.sgd_image(q.m, off, rs, -64, 64, 0.125, F32)
    got = img.copy()
    got[su.SGD_PAD + off - 1] += 1.0
    assert first_mismatch(got, img.astype(F64)) == (su.SGD_PAD + off - 1,)
    assert (q.m1 != q.m).mean() > 0.9 and (q.w1 != q.w).mean() > 0.9


def test_a_dropped_tile_column_of_a_transpose_is_a_mismatch_there():
    for case in su.tr_cases():
        batch, r, c, in_ld, out_ld, ibs, obs = case
        vals = su.tr_values(case, batch, True)
        src, dst = su.tr_images(case, batch, vals, np.nan, su.SENTINEL, F16)
        assert np.isnan(src).sum() == src.size - batch * r * c and (dst != su.SENTINEL).sum() <= batch * r * c
        assert np.array_equal(dst[:c * out_ld].reshape(c, out_ld)[:, :r], vals[0].T)
        col = min(c, 32) - 1                                          # the last column of the first 32 x 32 tile
        got = dst.astype(F16)
        got[col * out_ld:col * out_ld + min(r, 32)] = su.SENTINEL     # ... is row `col` of the output
        assert first_mismatch(got, dst) == (col * out_ld,), case
        # a write into a spare lane of the output pitch is one too
        if out_ld > r:
            got = dst.astype(F16)
            got[r] = 0.0
            assert first_mismatch(got, dst) == (r,)


def test_nonzero_padding_columns_of_a_transposed_weight_are_a_mismatch_there():
    for shape in su.WT_SHAPES:
        O, T, I, Opad = shape
        q = su.wt_problem(shape)
        assert q.wt.shape == (I, T, Opad) and (q.wt[:, :, O:] == 0).all() and np.array_equal(q.wt[:, :, :O], q.w.transpose(2, 1, 0))
        if Opad > O:
            got = q.wt.astype(F16)
            got[:, :, O:] = su.SENTINEL
            assert first_mismatch(got, q.wt) == (0, 0, O)
