# CPU-only checks of the exact SUMMA test method (tests/_exact_summa.py):
# the padded shard images reassemble to the global operands, the float64
# reference is exact (pinned against an int64 matmul), the case table
# holds what the GPU module is meant to cover, and the panel count the
# GPU test expects of gemm_launches is what the library plans.
import numpy as np
import pytest

import _exact
import _exact_summa as S
from marlin_amd import engine as E

CASES = S.virtual_cases()


def test_case_table_covers_the_required_cells():
    have = set(CASES)
    assert len(have) == len(CASES)
    for fp32 in (0, 1):
        for pr, pc in S.GRIDS:
            for shape in S.SHAPES:
                assert S.SummaCase(fp32, pr, pc, *shape, 48) in have
        for pr, pc in S.WIDTH_GRIDS:
            for kb in S.WIDTHS:
                assert S.SummaCase(fp32, pr, pc, *S.SHAPES[0], kb) in have
    for c in CASES:
        assert c.k <= (_exact.F32_KMAX if c.fp32 else _exact.F64_KMAX)
    for fp32, (m, k, n) in S.REAL_SHAPES.items():
        assert k <= (_exact.F32_KMAX if fp32 else _exact.F64_KMAX)
    # the edges the shapes were chosen for really exist in the table
    assert any(S.Geometry(c, c.pr - 1, 0).mi == 0 for c in CASES)
    assert any(E.slab_len(c.k, c.pr, c.pr - 1) == 0 for c in CASES)
    assert any(E.slab_off(c.k, c.pr, 1) % 16 for c in CASES if c.pr > 1)
    # the fp64 real-entry shape takes two panels at the default width
    assert len(E.plan_panels(S.REAL_SHAPES[0][1], 1, 1, 2048)) == 2


@pytest.mark.parametrize(
    "fp32,shape",
    [(f, s) for f in (0, 1) for s in S.SHAPES]
    + sorted(S.REAL_SHAPES.items()),
    ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"t{v}")
def test_float64_reference_is_exact_vs_int64(fp32, shape):
    m, k, n = shape
    a, b, ref, qa, qb = S.summa_inputs(fp32, m, k, n)
    exact = qa @ qb                       # int64: |q1*q2|*K <= 2^50
    scale = 1.0 if fp32 else 2.0 ** (-2 * _exact.F64_QBITS)
    np.testing.assert_array_equal(ref, exact.astype(np.float64) * scale)
    np.testing.assert_array_equal(exact.astype(np.float64).astype(np.int64),
                                  exact)


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_shards_reassemble_and_launch_counts(case):
    c = case
    dt = _exact.dtype_of(c.fp32)
    sent = _exact.NAN_BITS[dt]
    a, b, ref = S.summa_inputs(c.fp32, c.m, c.k, c.n)[:3]
    A = np.full((c.m, c.k), np.nan)
    B = np.full((c.k, c.n), np.nan)
    C = np.full((c.m, c.n), np.nan)
    panels = E.plan_panels(c.k, c.pr, c.pc, c.kb)
    assert panels[0][0] == 0 and panels[-1][1] == c.k
    assert all(0 < k1 - k0 <= c.kb for k0, k1, _, _ in panels)
    for i in range(c.pr):
        for j in range(c.pc):
            g = S.Geometry(c, i, j)
            kaj, kao = E.slab_len(c.k, c.pc, j), E.slab_off(c.k, c.pc, j)
            kbi, kbo = E.slab_len(c.k, c.pr, i), E.slab_off(c.k, c.pr, i)
            sa, sb = S.a_shard(c, i, j), S.b_shard(c, i, j)
            assert (sa is None) == (g.mi == 0 or kaj == 0)
            assert (sb is None) == (kbi == 0 or g.nj == 0)
            if sa is not None:
                assert sa.shape == (S.roundup(g.mi, 128), kaj + 1)
                assert sa.dtype == dt and sa.flags.f_contiguous
                A[g.mo:g.mo + g.mi, kao:kao + kaj] = sa[:g.mi, :kaj]
                assert (sa[g.mi:, :kaj] == 0).all()            # pad rows 0
                assert (_exact._bits(sa[:, kaj]) == sent).all()  # guard
            if sb is not None:
                assert sb.shape == (S.roundup(kbi, 16), g.nj + 1)
                assert sb.dtype == dt and sb.flags.f_contiguous
                B[kbo:kbo + kbi, g.no:g.no + g.nj] = sb[:kbi, :g.nj]
                assert (_exact._bits(sb[kbi:, :]) == sent).all()
                assert (_exact._bits(sb[:, g.nj]) == sent).all()
            cimg = S.c_image(c, g)
            assert (_exact._bits(cimg) == sent).all()
            want = 0 if g.empty else len(panels)
            assert S.expected_launches(c, i, j) == want
            if g.empty:
                continue
            assert cimg.shape == (g.mip, g.njp + 1)
            C[g.mo:g.mo + g.mi, g.no:g.no + g.nj] = S.ref_block(c, g)
            # the checker accepts the ideal image and sees each defect
            ideal = cimg.copy(order="F")
            ideal[:, :g.njp] = 0
            ideal[:g.mi, :g.nj] = S.ref_block(c, g)
            res = S.check_c_image(ideal, g.mi, g.nj, S.ref_block(c, g), sent)
            assert res == {"ok": True, "first_bad": None,
                           "sentinel_inside": False, "pad_ok": True,
                           "pad_rows_zero": True, "pad_cols_zero": True}
            if g.nj < g.njp:
                bad = ideal.copy(order="F")
                bad[0, g.njp - 1] = np.nan
                assert not S.check_c_image(bad, g.mi, g.nj, S.ref_block(c, g),
                                           sent)["pad_cols_zero"]
            if g.mi < g.mip:
                bad = ideal.copy(order="F")
                bad[g.mip - 1, 0] = 1
                assert not S.check_c_image(bad, g.mi, g.nj, S.ref_block(c, g),
                                           sent)["pad_rows_zero"]
            bad = ideal.copy(order="F")
            bad[g.mi - 1, g.nj - 1] += 1
            r = S.check_c_image(bad, g.mi, g.nj, S.ref_block(c, g), sent)
            assert not r["ok"] and r["first_bad"] == [g.mi - 1, g.nj - 1]
            bad = ideal.copy(order="F")
            bad[0, g.njp] = 0
            assert not S.check_c_image(bad, g.mi, g.nj, S.ref_block(c, g),
                                       sent)["pad_ok"]
    np.testing.assert_array_equal(A, a.astype(np.float64))
    np.testing.assert_array_equal(B, b.astype(np.float64))
    np.testing.assert_array_equal(C, ref)


def test_knob_child_launch_count():
    # what the MARLIN_SUMMA_KB=40 child must report for every entry
    panels = E.plan_panels(S.KNOB_SHAPE[1], 1, 1, S.KNOB_KB)
    assert len(panels) == -(-S.KNOB_SHAPE[1] // S.KNOB_KB) == 13
    assert len(E.plan_panels(S.KNOB_SHAPE[1], 1, 1, 2048)) == 1
