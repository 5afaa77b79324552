# The consumers of the grouped GEMM entry: blocked inverse / LU / Cholesky
# (marlin_amd/linalg.py) and BlockMatrix.multiply(BlockMatrix). Each batch
# of independent block products is one grouped launch; the per-product
# loop stays reachable (grouped=False, BlockMatrix._multiply_tile_chain)
# and must give the same raw bits, because every C tile runs the k-loop
# the plain entry runs.
import numpy as np
import pytest

from _linalg_cases import lu_residual, shuffled_dominant
from marlin_amd import Engine, DenseVecMatrix
from oracle import gen_matrix

pytestmark = pytest.mark.gpu

SIZES = [(300, 96), (517, 128)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))


def _well_conditioned(n, seed):
    return gen_matrix(n, n, seed=seed) + n * np.eye(n)


def _both(eng, run):
    """run(grouped) for the loop arm, then the grouped arm; the grouped
    arm must have gone through grouped launches of more than one
    problem."""
    loop = run(False)
    grouped = run(True)
    assert eng.last_gemm_group()[0] > 1
    return loop, grouped


@pytest.mark.parametrize("n,base", SIZES)
def test_inverse_grouped_bits_equal_loop(eng, n, base):
    a = _well_conditioned(n, seed=n)
    loop, grouped = _both(eng, lambda g: DenseVecMatrix(a, engine=eng).inverse(
        mode="dist", base_size=base, grouped=g).toBreeze())
    _bits_equal(grouped, loop)
    assert np.max(np.abs(a @ grouped - np.eye(n))) < 1e-9


@pytest.mark.parametrize("n,base", SIZES)
def test_lu_grouped_bits_equal_loop(eng, n, base):
    a = _well_conditioned(n, seed=1000 + n)

    def run(g):
        blk, p = DenseVecMatrix(a, engine=eng).luDecompose(
            mode="dist", base_size=base, grouped=g)
        return blk.toBreeze(), p
    (lu0, p0), (lu1, p1) = _both(eng, run)
    _bits_equal(lu1, lu0)
    np.testing.assert_array_equal(p1, p0)
    L = np.tril(lu1, -1) + np.eye(n)
    rel = np.max(np.abs(a[p1, :] - L @ np.triu(lu1))) / np.max(np.abs(a))
    assert rel < 1e-10, rel


@pytest.mark.parametrize("n,base", [(300, 96), (64, 16)])
def test_lu_pivoting_grouped_bits_equal_loop(eng, n, base):
    # an input on which p_array is not the identity (rows shuffled inside
    # each block row): L^-1 P feeds the batches of both arms
    a, src = shuffled_dominant(n, base)

    def run(g):
        blk, p = DenseVecMatrix(a, engine=eng).luDecompose(
            mode="dist", base_size=base, grouped=g)
        return blk.toBreeze(), p
    (lu0, p0), (lu1, p1) = _both(eng, run)
    _bits_equal(lu1, lu0)
    np.testing.assert_array_equal(p1, p0)
    assert (p1 != np.arange(n)).any()
    np.testing.assert_array_equal(src[p1], np.arange(n))
    rel = lu_residual(a, lu1, p1)
    assert rel < 1e-10, rel


@pytest.mark.parametrize("n,base", SIZES)
def test_cholesky_grouped_bits_equal_loop(eng, n, base):
    r = gen_matrix(n, n, seed=2000 + n)
    a = (r + r.T) / 2 + n * np.eye(n)
    loop, grouped = _both(
        eng, lambda g: DenseVecMatrix(a, engine=eng).choleskyDecompose(
            mode="dist", base_size=base, grouped=g).toBreeze())
    _bits_equal(grouped, loop)
    rel = np.max(np.abs(grouped @ grouped.T - a)) / np.max(np.abs(a))
    assert rel < 1e-12, rel


def test_block_multiply_grouped_bits_equal_tile_chain(eng):
    # 300 x 200 · 200 x 260 in 3 x 2 and 2 x 3 blocks: the problems of one
    # grouped call differ in shape (ragged last blocks)
    a = gen_matrix(300, 200, seed=0xB10C)
    b = gen_matrix(200, 260, seed=0xB10D)
    A = DenseVecMatrix(a, engine=eng).toBlockMatrix(3, 2)
    B = DenseVecMatrix(b, engine=eng).toBlockMatrix(2, 3)
    got = A.multiply(B)
    assert eng.last_gemm_group()[0] == A.numBlksByRow() * B.numBlksByCol() > 1
    chain = A._multiply_tile_chain(B)
    assert set(got._blocks) == set(chain._blocks)
    for k in chain._blocks:
        _bits_equal(got._blocks[k], chain._blocks[k])
    np.testing.assert_allclose(got.toBreeze(), a @ b, rtol=1e-12, atol=0)


def test_block_multiply_golden_4x4(eng):
    m4 = np.array([[0., 1, 2, 3], [2, 3, 4, 5], [3, 2, 1, 0], [1, 1, 1, 1]])
    c4 = np.array([[11., 10, 9, 8], [23, 24, 25, 26], [7, 11, 15, 19],
                   [6, 7, 8, 9]])
    blk = DenseVecMatrix(m4, engine=eng).toBlockMatrix(2, 2)
    got = blk.multiply(blk)
    assert eng.last_gemm_group() == (4, 4)
    chain = blk._multiply_tile_chain(blk)
    for k in chain._blocks:
        _bits_equal(got._blocks[k], chain._blocks[k])
    np.testing.assert_array_equal(got.toBreeze(), c4)
    assert np.allclose(got.toBreeze(), m4 @ m4)
