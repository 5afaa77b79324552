# The consumers of the device triangular solve on the GPU:
#   - cholesky_decompose(panel="trsm"): the factor reproduces A, the solve
#     entry is what produced the panels, and the default panel="inverse"
#     still returns the bits it returned before the argument existed
#     (tests/golden/chol300_inverse_parent.json, recorded from the commit
#     that precedes the triangular solve);
#   - DenseVecMatrix.solve / lu_solve: normwise backward error against
#     numpy.linalg.solve on the same system.
import hashlib
import json
import os

import numpy as np
import pytest

from _linalg_cases import shuffled_dominant
from marlin_amd import DenseVecMatrix, Engine
from oracle import gen_matrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chol300_inverse_parent.json")
N, BASE = 300, 128


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def trsm_calls(eng):
    """Every Engine.trsm_raw call of the test: ((n, r, flags...), mx_stats
    right after it)."""
    calls = []
    orig = eng.trsm_raw

    def spy(n, r, *args, **kw):
        rc = orig(n, r, *args, **kw)
        calls.append(((n, r) + tuple(args[4:]) + tuple(sorted(kw.items())),
                      eng.stats()))
        return rc
    eng.trsm_raw = spy
    yield calls
    del eng.trsm_raw


def spd(n):
    r = gen_matrix(n, n, seed=2000 + n)      # test_gpu_linalg.py's input
    return (r + r.T) / 2 + n * np.eye(n)


def test_cholesky_trsm_panel(eng, trsm_calls):
    a = spd(N)
    L = DenseVecMatrix(a, engine=eng).choleskyDecompose(
        mode="dist", base_size=BASE, panel="trsm").toBreeze()
    assert np.allclose(np.triu(L, 1), 0)
    rel = np.max(np.abs(L @ L.T - a)) / np.max(np.abs(a))
    assert rel < 1e-12, rel                  # test_cholesky_dist_route's bound
    # three block columns of 100: two column panels, each ONE right-side
    # solve over all the blocks below the diagonal, and mx_stats shows it
    assert [c[0][:2] for c in trsm_calls] == [(100, 256), (100, 128)]
    for (n, r, *_), st in trsm_calls:
        assert st["flops"] == float(n) * n * r
        assert st["gemm_launches"] == 0      # one diagonal block: no update
    # the trailing update of the last step is a grouped table of one
    assert eng.last_gemm_group()[0] == 1


def test_cholesky_inverse_panel_keeps_its_bits(eng, trsm_calls):
    a = spd(N)
    dvm = DenseVecMatrix(a, engine=eng)
    L0 = dvm.choleskyDecompose(mode="dist", base_size=BASE).toBreeze()
    L1 = dvm.choleskyDecompose(mode="dist", base_size=BASE,
                               panel="inverse").toBreeze()
    assert trsm_calls == []                  # the default does not solve
    np.testing.assert_array_equal(L0.view(np.uint64), L1.view(np.uint64))
    with open(GOLDEN) as f:
        gold = json.load(f)
    assert gold["n"] == N and gold["base_size"] == BASE
    digest = hashlib.sha256(np.ascontiguousarray(L0).tobytes()).hexdigest()
    assert digest == gold["sha256"], "panel='inverse' no longer returns " \
        "the bits of the commit before the triangular solve"


# ---------------------------------------------------------------------------
def dominant(n):
    return gen_matrix(n, n, seed=7000 + n) + n * np.eye(n)


def backward_error(a, x, b):
    """Normwise eta = ||A x - b|| / (||A|| ||x|| + ||b||), Frobenius norms,
    the residual evaluated in np.longdouble."""
    ld = np.longdouble
    res = a.astype(ld) @ x.astype(ld) - b.astype(ld)
    nrm = lambda v: float(np.sqrt(np.sum(np.square(v.astype(ld)))))
    return nrm(res) / (nrm(a) * nrm(x) + nrm(b))


SYSTEMS = {"dominant": lambda: dominant(N),
           "rows-shuffled": lambda: shuffled_dominant(N, BASE)[0]}


@pytest.mark.parametrize("cols", [None, 3], ids=["vector", "3-columns"])
@pytest.mark.parametrize("mode,base", [("dist", BASE), ("local", 1000)])
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_solve_backward_error(eng, trsm_calls, system, mode, base, cols):
    a = SYSTEMS[system]()
    rng = np.random.RandomState(11)
    b = rng.uniform(-1, 1, size=N if cols is None else (N, cols))
    x = DenseVecMatrix(a, engine=eng).solve(b, mode=mode, base_size=base)
    assert x.shape == b.shape
    # the packed factor read twice on the left: unit-lower, then upper
    assert len(trsm_calls) == 2
    for (n, r, *_), st in trsm_calls:
        assert (n, r) == (N, 128) and st["flops"] == float(N) * N * 128
        assert st["gemm_launches"] == 2      # three diagonal blocks
    u = 2.0 ** -53
    eta = backward_error(a, x, b)
    eta_np = backward_error(a, np.linalg.solve(a, b), b)
    print(f"solve {system} {mode} {'vector' if cols is None else cols}: "
          f"eta = {eta:.3e}, numpy eta = {eta_np:.3e}, "
          f"ratio to max(numpy, u) = {eta / max(eta_np, u):.2f}")
    # the margin of 16 is for blockwise pivoting and blocked accumulation
    assert eta <= 16 * max(eta_np, u), (eta, eta_np)
