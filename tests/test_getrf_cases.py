# The inputs of the LU factorisation tests, proven on the CPU before they
# reach the GPU (tests/_getrf_cases.py states the claim): the numpy
# restatement of the block-pivoted elimination returns the known factors and
# permutation bit for bit in fp32, fp64 and longdouble alike, with a unique
# maximum at every step of the exact group, exactly one tie in the tie case
# and exactly the intended zero pivot in the other.
import numpy as np
import pytest

import _getrf_cases as GC

TYPES = [np.float32, np.float64, np.longdouble]


def _same(got, want):
    return got.shape == want.shape and bool((got == want).all())


@pytest.mark.parametrize("n", GC.ORDERS)
def test_exact_inputs_factor_exactly(n):
    a, packed, p = GC.exact_problem(n)
    # A itself is exact in fp32: nothing is lost by the cast
    assert _same(a.astype(np.float32).astype(np.float64), a)
    assert np.abs(a).max() < 2 * n * 4
    for dt in TYPES:
        ties = []
        lu, piv, info = GC.block_lu(a.astype(dt), tie_cols=ties)
        assert info == 0 and ties == []
        assert _same(lu.astype(np.float64), packed), dt
        np.testing.assert_array_equal(piv, p)
    # P maps each 128-block to itself and is a permutation
    np.testing.assert_array_equal(p // GC.W, np.arange(n) // GC.W)
    np.testing.assert_array_equal(np.sort(p), np.arange(n))
    if n > 1:
        assert (p != np.arange(n)).any()
    L = np.tril(packed, -1) + np.eye(n)
    np.testing.assert_array_equal(a[p, :], L @ np.triu(packed))


def test_exact_result_does_not_depend_on_the_block_width():
    # blocking changes which rows are candidates, not the exact arithmetic:
    # with the permutation inside 4-blocks, widths 4 and 128 agree
    rng = np.random.RandomState(5)
    L, U = GC._factors(13, rng)
    a, packed, p = GC._assemble(L, U, GC.block_perm(13, rng, w=4))
    for w in (4, 128):
        lu, piv, info = GC.block_lu(a, w=w)
        assert info == 0 and _same(lu, packed)
        np.testing.assert_array_equal(piv, p)


def test_tie_case_has_one_tie_and_the_lowest_row_wins():
    a, packed, p = GC.tie_problem()
    c = GC.TIE_COL
    assert np.sum(np.abs(packed[c + 1:, c]) == 1) == 3
    for dt in TYPES:
        ties = []
        lu, piv, info = GC.block_lu(a.astype(dt), tie_cols=ties)
        assert info == 0 and ties == [c]
        assert _same(lu.astype(np.float64), packed)
        np.testing.assert_array_equal(piv, p)
    # four candidates tie, and the intended row is the lowest of them: any
    # other rule picks another row
    pos = GC.positions_at(p, c)
    at = int(np.nonzero(pos == c)[0][0])
    tied = [r for r in range(c, GC.W)
            if pos[r] == c or abs(packed[pos[r], c]) == 1]
    assert tied[0] == at and len(tied) == 4


def test_zero_pivot_case():
    a, packed, p = GC.zero_pivot_problem()
    j = GC.ZERO_COL - 1
    assert packed[j, j] == 0 and not packed[j + 1:, j].any()
    for dt in (np.float32, np.float64):
        lu, piv, info = GC.block_lu(a.astype(dt))
        assert info == GC.ZERO_COL
        # block 0 goes on exactly; the columns before the zero pivot are
        # the known factors in every row
        assert _same(lu[:, :j].astype(np.float64), packed[:, :j])
        assert _same(lu[:GC.W, :GC.W].astype(np.float64), packed[:GC.W, :GC.W])
        np.testing.assert_array_equal(piv, p)


def test_block_lu_passes_over_nan_and_reports_first_zero():
    a = np.eye(5)
    a[0, 0] = np.nan
    a[3, 0] = 1e-300
    lu, piv, info = GC.block_lu(a, w=4)
    assert piv[0] == 3 and info == 0
    z = np.diag([1.0, 0, 2, 0, 3])
    lu, piv, info = GC.block_lu(z, w=4)
    assert info == 2 and _same(lu, z)
    np.testing.assert_array_equal(piv, np.arange(5))


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("n", [129, 300])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_rounding_inputs_meet_the_bound_on_the_host(fp32, n, shuffled):
    a, src = GC.rounding_problem(fp32, n, shuffled)
    lu, piv, info = GC.block_lu(a)
    assert info == 0
    # the dominant diagonal is the pivot: the shuffle is undone
    np.testing.assert_array_equal(src[piv], np.arange(n))
    assert shuffled == bool((piv != np.arange(n)).any())
    assert GC.residual_ratio(fp32, a, lu, piv) <= 1.0
