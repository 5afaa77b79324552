# The consumers of the device LU factorisation on the GPU, n = 300 (three
# diagonal blocks, the last ragged):
#   - lu_decompose(panel="device"): A[p] == L U to the tolerance the LU test
#     of mode="dist" uses (test_gpu_linalg.py);
#   - DeviceLU.solve, twice on one factor, and solve(factor="device"):
#     normwise backward error eta <= 16 max(eta_ref, u), eta as in
#     test_gpu_trsm_consumers.py::test_solve_backward_error and with its
#     margin, eta_ref from a host solve through the numpy restatement of the
#     same 128-block pivoting in the same element type;
#   - solve() without the argument returns the bytes of factor="host";
#   - the factor's image is released once: a second free() is a no-op (the
#     engine keeps no allocation count to compare).
import numpy as np
import pytest

import _getrf_cases as GC
from _linalg_cases import lu_residual
from marlin_amd import DenseVecMatrix, Engine
from marlin_amd.linalg import lu_factor_device
from oracle import gen_matrix

pytestmark = pytest.mark.gpu

N = 300


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def dominant(n):
    return gen_matrix(n, n, seed=7000 + n) + n * np.eye(n)


def shuffled(n):
    """dominant(n) with its rows shuffled inside each 128-block: what
    pivoting inside the device's diagonal blocks can undo."""
    src = GC.block_perm(n, np.random.RandomState(7100 + n))
    return np.asfortranarray(dominant(n)[src, :])


SYSTEMS = {"dominant": lambda: dominant(N), "rows-shuffled": lambda: shuffled(N)}


def backward_error(a, x, b):
    """Normwise eta = ||A x - b|| / (||A|| ||x|| + ||b||), Frobenius norms,
    the residual evaluated in np.longdouble."""
    ld = np.longdouble
    res = a.astype(ld) @ x.astype(ld) - b.astype(ld)
    nrm = lambda v: float(np.sqrt(np.sum(np.square(v.astype(ld)))))
    return nrm(res) / (nrm(a) * nrm(x) + nrm(b))


def _meets_bound(what, a, x, b, fp32=False):
    dt = np.float32 if fp32 else np.float64
    u = 2.0 ** (-24 if fp32 else -53)
    at, bt = a.astype(dt), b.astype(dt)
    eta = backward_error(at, x, bt)
    eta_ref = backward_error(at, GC.block_lu_solve(at, bt), bt)
    print(f"getrf solve {what}: eta = {eta:.3e}, host block-pivoted eta = "
          f"{eta_ref:.3e}, ratio to max(ref, u) = {eta / max(eta_ref, u):.2f}")
    assert eta <= 16 * max(eta_ref, u), (what, eta, eta_ref)


@pytest.mark.parametrize("system", list(SYSTEMS))
def test_lu_decompose_device_panel(eng, system):
    a = SYSTEMS[system]()
    blk, p_array = DenseVecMatrix(a, engine=eng).luDecompose(
        mode="dist", base_size=96, panel="device")
    lu = blk.toBreeze()
    assert lu.shape == (N, N) and p_array.shape == (N,)
    np.testing.assert_array_equal(p_array // 128, np.arange(N) // 128)
    if system == "rows-shuffled":
        assert (p_array != np.arange(N)).any()
    rel = lu_residual(a, lu, p_array)
    assert rel < 1e-10, rel


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_device_lu_solves_twice_on_one_factor(eng, system, fp32):
    a = SYSTEMS[system]()
    rng = np.random.RandomState(11)
    with lu_factor_device(DenseVecMatrix(a, engine=eng), fp32=fp32) as f:
        for cols in (None, 3):
            b = rng.uniform(-1, 1, size=N if cols is None else (N, cols))
            x = f.solve(b)
            assert x.shape == b.shape
            _meets_bound(f"DeviceLU {system} {'f32' if fp32 else 'f64'} "
                         f"{'vector' if cols is None else cols}", a, x, b,
                         fp32)
        lu, p = f.download()
        assert lu.shape == (N, N) and p is f.p_array
    assert f._image is None
    f.free()                                 # a second free is a no-op
    with pytest.raises(ValueError):
        f.solve(np.ones(N))


@pytest.mark.parametrize("cols", [None, 3], ids=["vector", "3-columns"])
@pytest.mark.parametrize("system", list(SYSTEMS))
def test_solve_device_factor(eng, system, cols):
    a = SYSTEMS[system]()
    rng = np.random.RandomState(11)
    b = rng.uniform(-1, 1, size=N if cols is None else (N, cols))
    x = DenseVecMatrix(a, engine=eng).solve(b, factor="device")
    assert x.shape == b.shape
    _meets_bound(f"solve(factor='device') {system} "
                 f"{'vector' if cols is None else cols}", a, x, b)


def test_solve_default_is_the_host_factor(eng):
    a = SYSTEMS["rows-shuffled"]()
    b = np.random.RandomState(12).uniform(-1, 1, size=(N, 2))
    dvm = DenseVecMatrix(a, engine=eng)
    x0 = dvm.solve(b, mode="dist", base_size=128)
    x1 = dvm.solve(b, mode="dist", base_size=128, factor="host")
    np.testing.assert_array_equal(x0.view(np.uint64), x1.view(np.uint64))
