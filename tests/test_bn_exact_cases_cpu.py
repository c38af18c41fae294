"""CPU: the case generator, the conditions and the comparisons of the exact BatchNorm tests (bn_exact_util.py; DESIGN.md "Exact
BatchNorm tests").  Nothing here launches a kernel: the generator meets every seam of bn_grid for every channel count, the
restated bn_grid agrees with the library's own (through sn_bn_workspace_bytes) and with values worked out by hand, every case
satisfies the conditions its zero tolerance rests on, and every defect the GPU test is there for -- a row lost or counted twice,
a chunk of the second slab not written, an edge element masked the wrong way, `accumulate` read after the store -- is caught by the
very comparison the GPU test makes."""
import numpy as np
import pytest

import bn_exact_util as bx


def test_bn_grid_agrees_with_values_worked_out_by_hand():
    # (M, C) -> (row blocks, slabs, rows per block): DESIGN.md section 18's table
    for (M, C), want in {(2049, 2048): (228, 1, 9), (20480, 1024): (512, 1, 40), (33000, 256): (459, 1, 72),
                         (2049, 256): (33, 1, 64), (257, 1024): (17, 1, 16), (2048, 8): (1, 1, 2048), (2049, 8): (2, 1, 1280),
                         (681, 24): (2, 1, 425), (1024, 2056): (128, 2, 8), (8193, 1024): (456, 1, 18)}.items():
        assert bx.bn_grid(M, C) == want, ((M, C), bx.bn_grid(M, C), want)
    assert [bx.bn_rpp(C) for C in bx.C_EDGES] == [256, 128, 85, 51, 28, 21, 8, 2, 1, 1, 1]
    assert [bx.bn_reduce_cap(C) for C in (8, 256, 1024, 2048, 2056, 2560)] == [512, 512, 512, 256, 256, 256]
    assert bx.bn_grid(65536, 2048, bx.DX_CAP)[0] == 8192 and bx.bn_grid(65537, 2048, bx.DX_CAP)[2] == 9      # the out-of-scope cap


def test_bn_grid_agrees_with_the_library():
    """sn_bn_workspace_bytes = align256(4 * 2C * (blocks + 1)): with 2C floats per block a multiple of 256 bytes (C >= 32) this
    fixes the library's block count; below that it fixes it to within the alignment"""
    from sniper_amd import build as hipbuild
    hipbuild.build(verbose=False)
    from sniper_amd._lib import lib
    raw = lib().raw('sn_bn_workspace_bytes')
    n = 0
    for C in bx.C_EDGES:
        for M in set(bx.m_edges(C)) | {bx.bn_reduce_cap(C) * 8 * bx.bn_rpp(C), 20480, 65536}:
            assert raw(M, C) == bx.workspace_bytes(M, C), (M, C, raw(M, C), bx.workspace_bytes(M, C))
            n += 1
    assert n >= 120


@pytest.mark.parametrize('C', bx.C_EDGES)
def test_the_generator_meets_every_seam(C):
    rpp, cap, s = bx.bn_rpp(C), bx.bn_reduce_cap(C), bx.seams(C)
    Ms = bx.m_edges(C)
    assert len(Ms) <= 15 and all((M, C) in bx.cases() for M in Ms)
    assert {1, 3, rpp, rpp + 1} <= set(Ms) and (rpp == 1 or rpp - 1 in Ms)
    assert any(M < rpp for M in Ms) or rpp == 1                                          # fewer rows than row lanes
    assert any(bx.bn_grid(M, C)[2] < bx.BN_UNROLL * rpp for M in Ms)                     # only the remainder loop runs
    assert any(bx.bn_grid(M, C) == (1, bx.div_up(C // 8, 256), bx.BN_UNROLL * rpp) and M == bx.BN_UNROLL * rpp for M in Ms)
    one = max(M for M in Ms if bx.bn_grid(M, C)[0] == 1)
    assert bx.bn_grid(one + 1, C)[0] == 2 and one + 1 in Ms and one == 8 * rpp          # the largest single block, and one more
    assert any(bx.bn_grid(M, C)[0] > 1 and bx.last_rows(M, C) == 1 for M in Ms)          # a last block of one row
    assert any(bx.is_pow2(M) and M >= 1024 for M in Ms)
    if C in bx.CAP_CS:
        M = s['first M beyond the reduce cap']
        assert bx.div_up(M - 1, 8 * rpp) == cap and bx.bn_grid(M - 1, C)[2] == 8 * rpp and bx.bn_grid(M, C)[2] > 8 * rpp
        assert bx.bn_grid(M, C)[0] <= cap
    assert max(M * C for M in Ms) * 2 <= 17.5e6                                          # bytes of the largest fp16 operand
    assert all(bx.bn_grid(M, C, bx.DX_CAP)[0] < bx.DX_CAP for M in Ms)                   # (the dx cap: out of scope)
    assert bx.bn_grid(1024, C)[1] == (2 if C > 2048 else 1)


@pytest.mark.parametrize('C', bx.C_EDGES)
def test_conditions_hold_and_every_perturbation_is_caught(C):
    """per case: the conditions; then, with accumulate = acc, the reference as a correct kernel stores it passes the GPU test's
    comparison and each perturbed one fails it"""
    caught = {k: 0 for k in bx.PERTURBATIONS}
    edges = 0
    for i, (M, _) in enumerate(bx.cases(C)):
        q = bx.problem(M, C)
        assert bx.check_conditions(q)
        act = bx.ACTS[i % 3] if M > 4096 else None              # the largest cases: one activation each
        for a in bx.ACTS if act is None else (act,):
            r = bx.backward_ref(M, C, a)
            edges += int(r.edges.sum())
            dx, dg, db = bx.stored(q, r, q.acc)
            assert bx.backward_failures(q, r, dx, q.acc, dg, db, 'reference') == []
            dx, dg, db = bx.stored(q, r, None)
            assert bx.backward_failures(q, r, dx, None, dg, db, 'reference, no accumulate') == []
            for kind in bx.PERTURBATIONS:
                if kind == 'edge mask flipped' and not (r.edges & (q.dy != 0)).any():
                    continue                                     # (act 0 has no edge; a one-row case may have none with dy != 0)
                dx, dg, db, acc = bx.perturbed(q, a, kind)
                msgs = bx.backward_failures(q, r, dx, acc, dg, db, kind)
                assert msgs, ((M, C), a, kind, 'not caught')
                caught[kind] += 1
    n = len(bx.cases(C))
    assert edges > 0
    for kind, k in caught.items():
        assert k >= (n if kind == 'edge mask flipped' else 2 * n), (kind, k, n)


def test_forward_comparison_catches_a_lost_and_a_doubled_row():
    """sn_bn_stats' sums with one row missing or twice: save_mean differs on the bits at every M, the smallest case and the
    largest alike (the tolerance this replaces, rtol 1e-3, passes both)"""
    f32 = np.float32
    for (M, C) in ((3, 8), (1024, 96), (33000, 256), (2049, 2048), (57, 2560)):
        q = bx.problem(M, C)
        r = bx.forward_ref(q, 2e-5, 0.9, False)
        ok = bx.forward_failures(M, r, r.scale32 if bx.is_pow2(M) else r.scale.astype(f32), r.shift32 if bx.is_pow2(M) else r.shift.astype(f32),
                                 r.mean.astype(f32), r.invstd.astype(f32), r.run_mean.astype(f32), r.run_var.astype(f32), 'reference')
        assert ok == [], ok
        for w in (0.0, 2.0):
            row = M - 1
            s = r.sum + (w - 1.0) * q.x[row]
            bad = bx.compare_exact((s / M).astype(f32), r.mean, 'save_mean')
            assert bad, ((M, C), w)
        rel = np.abs((r.sum - q.x[M - 1]) / M - r.mean).max() / 2.6          # in standard deviations of x
        assert M < 1000 or rel < 1e-2                                        # ... what the old tolerance could not see


def test_ulp_helpers():
    assert bx.ulp16(1.0) == 2.0 ** -10 and bx.ulp16(1.9995) == 2.0 ** -10 and bx.ulp16(2.0) == 2.0 ** -9
    assert bx.ulp16(0.0) == 2.0 ** -24 and bx.ulp16(2.0 ** -14) == 2.0 ** -24 and bx.ulp16(-6.0) == 2.0 ** -8
    assert bx.ulp32(1.0) == 2.0 ** -23 and bx.ulp32(-0.75) == 2.0 ** -24
    assert bx.fits(0.5, np.float16) and not bx.fits(2049.0, np.float16) and not bx.fits(1.0 / 3, np.float32)
    part = bx.block_partials(np.arange(12.0).reshape(6, 2), 4)
    assert part.shape == (4, 2) and np.array_equal(part.sum(axis=0), [30.0, 36.0])
    assert np.array_equal(bx.block_partials(np.ones((3, 1)), 5).ravel(), [0, 1, 0, 1, 1])
