"""The exact convolution oracle checked without a GPU (conv_exact_util.py): the case generator is deterministic and covers
the tile edges pair by pair, every case meets the conditions the zero tolerance rests on, and the comparison the GPU tests use
sees a single dropped or doubled (pixel, tap, 8-channel chunk) contribution -- what the Gaussian tests' 1e-2 bounds cannot."""
import numpy as np

import conv_exact_util as cx


def test_generator_is_deterministic():
    first = cx.cases()
    cx.cases.cache_clear()
    second = cx.cases()
    assert first == second and len(set(first)) == len(first)
    assert cx.case_seed(first[0]) == cx.case_seed(tuple(first[0])) and cx.case_seed(first[0]) != cx.case_seed(first[1])


def test_generator_covers_every_pair_of_edges_within_the_size_cap():
    cs = cx.cases()
    assert 150 <= len(cs) <= 250, len(cs)
    mo, mg, oc, cg = set(), set(), set(), set()
    for case in cs:
        N, H, W, C, O, K, s, p, d = case
        Ho, Wo, M = cx.case_dims(case)
        assert Ho >= 1 and Wo >= 1 and M <= cx.MAX_PIXELS and C <= cx.MAX_CHANNELS and O <= cx.MAX_CHANNELS, case
        assert C % 8 == 0, case
        g = (K, s, p, d)
        mo.add((M, O)); mg.add((M, g)); oc.add((O, C)); cg.add((C, g))
    # the only pairs no shape realises: (3, 1, 2, 1) has Ho = H + 2 >= 3 and Wo >= 3, and 1, 127 and 257 have no two factors >= 3
    ring = (3, 1, 2, 1)
    assert cx.infeasible_pairs() == ((1, ring), (127, ring), (257, ring))
    for m in (1, 127, 257):
        assert not any(a >= 3 and b >= 3 for (_, a, b) in cx.factorisations(m))
    assert all((m, o) in mo for m in cx.M_EDGES for o in cx.COUT_EDGES)
    assert all((m, g) in mg for m in cx.M_EDGES for g in cx.GEOMS if (m, g) not in cx.infeasible_pairs())
    assert all((o, c) in oc for o in cx.COUT_EDGES for c in cx.CIN_EDGES)
    assert all((c, g) in cg for c in cx.CIN_EDGES for g in cx.GEOMS)


def test_generator_covers_row_lengths_images_and_stride_2_parities():
    cs = cx.cases()
    wide = [(c, cx.case_dims(c)) for c in cs if c[5] > 1]
    assert any(Wo < 32 for _, (Ho, Wo, M) in wide) and any(Wo == 32 for _, (Ho, Wo, M) in wide) and any(Wo == 33 for _, (Ho, Wo, M) in wide)
    assert any((c[0] * Ho * ((Wo + 31) // 32)) % 2 == 1 and c[0] * Ho * ((Wo + 31) // 32) > 1 for c, (Ho, Wo, M) in wide)
    # a row tile that straddles an image boundary: several images whose pixel count is no multiple of the smallest row tile
    assert sum(1 for c in cs if c[0] > 1 and (cx.case_dims(c)[0] * cx.case_dims(c)[1]) % 64 != 0 and cx.case_dims(c)[2] > 64) >= 10
    s2 = [c for c in cs if c[6] == 2]
    assert any(c[1] % 2 == 0 and c[2] % 2 == 0 for c in s2) and any(c[1] % 2 == 1 or c[2] % 2 == 1 for c in s2)
    for K in (1, 3, 5):          # ... each kernel size of a stride-2 geometry under both walks
        assert {(c[1] % 2 == 0 and c[2] % 2 == 0) for c in s2 if c[5] == K} == {True, False}, K


def test_every_case_meets_the_exactness_conditions():
    for case in cx.cases():
        q = cx.problem(case)
        cx.check_conditions(q)
        assert q.salt <= 2, (case, q.salt)
        # fp16 exactness of everything a kernel stores as fp16: the cast is the identity
        for name in ('x', 'w', 'dy', 'res', 'acc', 'bn_x', 'y', 'y_brr', 'dx', 'dx_acc'):
            a = getattr(q, name)
            assert np.array_equal(a.astype(np.float16).astype(np.float64), a), (case, name)
        for name in ('dw', 'dw0', 'y_q', 'bias', 'bias_q', 'bn_scale', 'bn_shift', 'bn_mean'):
            a = getattr(q, name)
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a), (case, name)
        pre = cx.rows_nhwc(q.bn_x) * q.bn_scale + q.bn_shift
        assert not np.any(pre == 0) and not np.any(pre == 6), case


def test_references_restate_the_convolution():
    """the float64 references against a direct numpy restatement of the definition (no torch), on a few small cases"""
    small = sorted(cx.cases(), key=lambda c: cx.case_dims(c)[2] * c[3] * c[4] * c[5] ** 2)[5:60:11]
    for case in small:
        N, H, W, C, O, K, s, p, d = case
        q = cx.problem(case)
        Ho, Wo, M = cx.case_dims(case)
        y, dx, dw = np.zeros_like(q.y), np.zeros_like(q.x), np.zeros_like(q.w)
        for n in range(N):
            for oy in range(Ho):
                for ox in range(Wo):
                    for kh in range(K):
                        for kw in range(K):
                            sy, sx = oy * s - p + kh * d, ox * s - p + kw * d
                            if 0 <= sy < H and 0 <= sx < W:
                                y[n, :, oy, ox] += q.w[:, :, kh, kw] @ q.x[n, :, sy, sx]
                                dx[n, :, sy, sx] += q.dy[n, :, oy, ox] @ q.w[:, :, kh, kw]
                                dw[:, :, kh, kw] += np.outer(q.dy[n, :, oy, ox], q.x[n, :, sy, sx])
        assert np.array_equal(y, q.y) and np.array_equal(dx, q.dx) and np.array_equal(dw, q.dw), case


def test_one_dropped_or_doubled_chunk_is_seen():
    """the sensitivity the zero tolerance buys: for a sample of cases, remove ONE (pixel, tap, 8-channel chunk) contribution from
    the forward result, or count it twice, and the comparison of the GPU tests reports a mismatch at that pixel, naming its tile"""
    rs = np.random.RandomState(0)
    cs = cx.cases()
    seen = 0
    for case in cs[::4]:
        N, H, W, C, O, K, s, p, d = case
        q = cx.problem(case)
        Ho, Wo, M = cx.case_dims(case)
        want = cx.rows_nhwc(q.y).astype(np.float16)
        assert cx.exact_equal(want, cx.rows_nhwc(q.y))
        for attempt in range(200):           # a contribution that exists: a tap inside the image, a chunk with a non-zero product
            pixel = (rs.randint(N), rs.randint(Ho), rs.randint(Wo))
            tap, chunk = (rs.randint(K), rs.randint(K)), rs.randint(C // 8)
            if not np.array_equal(cx.perturbed_forward(q, pixel, tap, chunk, 0.0), q.y):
                break
        else:
            raise AssertionError('no non-zero contribution found in %s' % (case,))
        for factor in (0.0, 2.0):
            wrong = cx.rows_nhwc(cx.perturbed_forward(q, pixel, tap, chunk, factor)).astype(np.float16)
            bad = cx.first_mismatch(wrong, cx.rows_nhwc(q.y))
            assert bad is not None and bad[0] == (pixel[0] * Ho + pixel[1]) * Wo + pixel[2], (case, pixel, tap, chunk, factor, bad)
            try:
                cx.assert_exact_rows(wrong, cx.rows_nhwc(q.y), 'sensitivity', Wo, Ho * Wo, (64, 128))
            except AssertionError as e:
                assert 'first row %d' % bad[0] in str(e) and 'tile (%d, %d)' % (bad[0] // 64, bad[1] // 128) in str(e), str(e)
            else:
                raise AssertionError('assert_exact_rows let a wrong result through')
            seen += 1
    assert seen >= 2 * 40


def test_guard_pitches():
    assert cx.pitch_of(72, 'dense') == (72, 0) and cx.pitch_of(65, 'dense') == (72, 0) and cx.pitch_of(65, 'packed') == (65, 0)
    assert cx.pitch_of(72, '+8') == (80, 0) and cx.pitch_of(72, '+24') == (96, 0) and cx.pitch_of(72, 'slice') == (152, 8)
    for C in (8, 42, 65, 130, 264):
        for kind in ('dense', '+8', '+24', 'slice'):
            pitch, off = cx.pitch_of(C, kind)
            assert pitch % 8 == 0 and off % 8 == 0 and off + C <= pitch
