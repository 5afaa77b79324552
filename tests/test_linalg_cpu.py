# The decomposition tier (marlin_amd/linalg.py) against a numpy stand-in
# for the engine: the block bookkeeping of lu_decompose, inverse and
# cholesky_decompose (which block is scaled by what, the perm loop, L^-1 P
# folded into the panel factor, the sub-diagonal permutation fix-up) runs
# on any machine. The LU inputs are the ones on which pivoting happens:
# every other LU input of the suite is diagonally dominant as given, so
# p_array is the identity there.
import numpy as np
import pytest

from _linalg_cases import NumpyEngine, lu_residual, shuffled_dominant
from marlin_amd import DenseVecMatrix
from oracle import gen_matrix

SHUFFLED = [(300, 96), (250, 64), (130, 128), (64, 16)]


@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "loop"])
@pytest.mark.parametrize("n,base", SHUFFLED)
def test_lu_undoes_a_shuffle_inside_each_block_row(n, base, grouped):
    a, src = shuffled_dominant(n, base)
    eng = NumpyEngine()
    blk, p_array = DenseVecMatrix(a, engine=eng).luDecompose(
        mode="dist", base_size=base, grouped=grouped)
    assert (p_array != np.arange(n)).any()             # pivoting happened
    np.testing.assert_array_equal(src[p_array], np.arange(n))
    rel = lu_residual(a, blk.toBreeze(), p_array)
    assert rel < 1e-10, rel
    assert (eng.grouped_calls > 0) == grouped
    assert all(h.freed for h in eng.live)              # nothing leaked


def test_lu_uniform_input_pivots_on_size():
    # no dominance at all: partial pivoting inside each diagonal block
    # chooses by magnitude (max|L| well above 1 across blocks)
    n, base = 130, 128
    a = gen_matrix(n, n, seed=0x130) - 0.5
    blk, p_array = DenseVecMatrix(a, engine=NumpyEngine()).luDecompose(
        mode="dist", base_size=base)
    assert (p_array != np.arange(n)).any()
    assert sorted(p_array) == list(range(n))
    rel = lu_residual(a, blk.toBreeze(), p_array)
    assert rel < 1e-10, rel


@pytest.mark.parametrize("n,base", SHUFFLED)
def test_inverse_of_shuffled_input(n, base):
    a, _ = shuffled_dominant(n, base)
    eng = NumpyEngine()
    inv = DenseVecMatrix(a, engine=eng).inverse(mode="dist",
                                                base_size=base).toBreeze()
    err = np.max(np.abs(a @ inv - np.eye(n)))
    assert err < 1e-9, err
    assert all(h.freed for h in eng.live)


@pytest.mark.parametrize("n,base", [(300, 96), (64, 16)])
def test_cholesky_blocked(n, base):
    r = gen_matrix(n, n, seed=2000 + n)
    a = (r + r.T) / 2 + n * np.eye(n)
    eng = NumpyEngine()
    L = DenseVecMatrix(a, engine=eng).choleskyDecompose(
        mode="dist", base_size=base).toBreeze()
    assert np.allclose(np.triu(L, 1), 0)
    rel = np.max(np.abs(L @ L.T - a)) / np.max(np.abs(a))
    assert rel < 1e-12, rel
    assert all(h.freed for h in eng.live)
