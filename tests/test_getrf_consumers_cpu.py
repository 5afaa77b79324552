# The consumers of the device LU factorisation without a GPU: the new
# arguments of lu_decompose / luDecompose / solve (their defaults take the
# path they took before, anything else is refused), and DeviceLU /
# lu_factor_device against a numpy stand-in for the part of Engine they use,
# so that the permutation of the right-hand side, the reuse of one factor,
# the release of the image and the zero-pivot error run on any machine.
import numpy as np
import pytest
import scipy.linalg

import _getrf_cases as GC
from marlin_amd import DenseVecMatrix
from marlin_amd.linalg import DeviceLU, lu_decompose, lu_factor_device
from oracle import gen_matrix


def dominant(n):
    return gen_matrix(n, n, seed=8100 + n) + n * np.eye(n)


def test_bogus_panel_and_factor_are_refused():
    dvm = DenseVecMatrix(dominant(6))
    with pytest.raises(ValueError, match="panel"):
        lu_decompose(dvm, mode="local", panel="bogus")
    with pytest.raises(ValueError, match="panel"):
        dvm.luDecompose(mode="local", panel="bogus")
    with pytest.raises(ValueError, match="factor"):
        dvm.solve(np.ones(6), mode="local", factor="bogus")


def test_host_panel_is_the_path_without_the_argument():
    a = dominant(40)[np.random.RandomState(3).permutation(40), :]
    dvm = DenseVecMatrix(a)
    blk0, p0 = dvm.luDecompose(mode="local")
    blk1, p1 = dvm.luDecompose(mode="local", panel="host")
    blk2, p2 = lu_decompose(dvm, "local", 1000, True, "host")
    for blk, p in ((blk1, p1), (blk2, p2)):
        np.testing.assert_array_equal(blk.toBreeze().view(np.uint64),
                                      blk0.toBreeze().view(np.uint64))
        np.testing.assert_array_equal(p, p0)


class _Image:
    def __init__(self, a, fp32):
        self.a = np.array(a, dtype=np.float32 if fp32 else np.float64,
                          order="F")
        self.m, self.n = self.a.shape
        self.fp32 = fp32
        self.freed = False

    def free(self):
        assert not self.freed, "freed twice"
        self.freed = True


class GetrfNumpyEngine:
    """upload / download, getrf_dd through the block-pivoted restatement,
    trsm_dd through scipy: what DeviceLU and lu_factor_device call."""

    def __init__(self):
        self.images = []

    def live(self):
        return sum(not im.freed for im in self.images)

    def upload_matrix(self, a, fp32=False):
        im = _Image(a, fp32)
        self.images.append(im)
        return im

    def download_matrix(self, dm):
        assert not dm.freed
        return dm.a.copy(order="F")

    def getrf_dd(self, A):
        assert not A.freed and A.m == A.n
        lu, piv, info = GC.block_lu(A.a)
        A.a[...] = lu
        return piv.astype(np.int64), info

    def trsm_dd(self, T, B, side="left", lower=True, trans=False,
                unit_diag=False):
        assert not (T.freed or B.freed) and side == "left" and not trans
        B.a[...] = scipy.linalg.solve_triangular(
            T.a, B.a, lower=lower, unit_diagonal=unit_diag)
        return B


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
def test_device_lu_solves_reuses_and_frees(fp32):
    n = 150
    a, _ = GC.rounding_problem(0, n, True)          # pivots have work to do
    eng = GetrfNumpyEngine()
    f = lu_factor_device(DenseVecMatrix(np.array(a), engine=eng), fp32=fp32)
    assert isinstance(f, DeviceLU) and eng.live() == 1
    assert f.p_array.dtype == np.int64 and (f.p_array != np.arange(n)).any()
    lu, p = f.download()
    L = np.tril(lu, -1) + np.eye(n)
    tol = 1e-4 if fp32 else 1e-12
    assert np.max(np.abs(a[p, :] - L @ np.triu(lu))) < tol * n
    rng = np.random.RandomState(4)
    for shape in (n, (n, 3)):                       # one factor, two solves
        b = rng.uniform(-1, 1, size=shape)
        x = f.solve(b)
        assert x.shape == b.shape
        assert x.dtype == (np.float32 if fp32 else np.float64)
        assert np.max(np.abs(a @ x - b)) < tol
        assert eng.live() == 1                      # only the factor remains
    with pytest.raises(ValueError, match="rows"):
        f.solve(np.ones(n + 1))
    f.free()
    assert eng.live() == 0
    f.free()                                        # a no-op
    with pytest.raises(ValueError, match="free"):
        f.solve(np.ones(n))
    with lu_factor_device(DenseVecMatrix(np.array(a), engine=eng)) as g:
        assert eng.live() == 1
    assert eng.live() == 0 and g._image is None


def test_device_paths_of_the_consumers():
    n = 150
    a, _ = GC.rounding_problem(0, n, True)
    a = np.array(a)
    eng = GetrfNumpyEngine()
    dvm = DenseVecMatrix(a, engine=eng)
    blk, p = dvm.luDecompose(mode="dist", base_size=7, panel="device")
    lu = blk.toBreeze()
    assert lu.shape == (n, n) and eng.live() == 0
    L = np.tril(lu, -1) + np.eye(n)
    assert np.max(np.abs(a[p, :] - L @ np.triu(lu))) < 1e-10
    b = np.random.RandomState(5).uniform(-1, 1, size=(n, 2))
    x = dvm.solve(b, factor="device")
    assert np.max(np.abs(a @ x - b)) < 1e-12 and eng.live() == 0


def test_zero_pivot_raises_and_releases_the_image():
    a, _, _ = GC.zero_pivot_problem()
    eng = GetrfNumpyEngine()
    with pytest.raises(np.linalg.LinAlgError, match=f"column {GC.ZERO_COL}"):
        lu_factor_device(DenseVecMatrix(np.array(a), engine=eng))
    assert len(eng.images) == 1 and eng.live() == 0
    with pytest.raises(ValueError, match="square"):
        lu_factor_device(DenseVecMatrix(np.ones((3, 4)), engine=eng))
