# The consumers of the device triangular solve without a GPU:
# cholesky_decompose(panel="trsm") and lu_solve / DenseVecMatrix.solve run
# against a numpy stand-in for the raw-buffer part of Engine they use, so
# the panel layout (stacked padded blocks, offsets of the trailing update),
# the permutation of the right-hand side and the padding run on any machine.
# The stand-in keeps flat buffers and honours offsets and pitches the way
# the C ABI does; its triangular solve reads only the referenced triangle.
import numpy as np
import pytest
import scipy.linalg

from marlin_amd import DenseVecMatrix, Engine
from marlin_amd.engine import DeviceMatrix
from marlin_amd.linalg import lu_solve
from oracle import gen_matrix


class RawNumpyEngine:
    OPS = Engine.OPS
    _SIDES = Engine._SIDES
    trsm_dd = Engine.trsm_dd

    def __init__(self):
        self.trsm_calls = []
        self.live = 0

    # -- buffers
    def alloc(self, nbytes):
        assert nbytes > 0 and nbytes % 8 == 0
        self.live += 1
        return np.full(nbytes // 8, np.nan)

    def free(self, buf):
        self.live -= 1

    def upload(self, buf, arr, nbytes):
        buf[:nbytes // 8] = np.asarray(arr).ravel(order="F")[:nbytes // 8]

    def download(self, arr, buf, nbytes):
        arr[...] = buf[:nbytes // 8].reshape(arr.shape, order="F")

    def upload_matrix(self, a, fp32=False):
        a = np.asarray(a, dtype=np.float64)
        m, n = a.shape
        pitch, ncap = (m + 127) // 128 * 128, (n + 127) // 128 * 128
        img = np.zeros((pitch, ncap), order="F")
        img[:m, :n] = a
        buf = self.alloc(img.nbytes)
        self.upload(buf, img, img.nbytes)
        return DeviceMatrix(self, buf, m, n, pitch, False)

    def download_matrix(self, dm):
        ncap = (dm.n + 127) // 128 * 128
        return dm.buf[:dm.pitch * ncap].reshape(
            (dm.pitch, ncap), order="F")[:dm.m, :dm.n].copy(order="F")

    @staticmethod
    def _view(buf, off, ld, rows, cols):
        assert off >= 0 and off + (cols - 1) * ld + rows <= buf.size
        return np.lib.stride_tricks.as_strided(
            buf[off:], shape=(rows, cols), strides=(8, 8 * ld))

    # -- the entries
    def trsm_raw(self, n, r, dT, ldt, dB, ldb, side=0, lower=1, trans=0,
                 unit_diag=0, fp32=False, check=True):
        assert not fp32 and r % 128 == 0 and dT is not dB
        self.trsm_calls.append((n, r, side, lower, trans, unit_diag))
        np_ = (n + 127) // 128 * 128
        assert ldt >= np_ and ldb >= (r if side else np_)
        t = self._view(dT, 0, ldt, np_, np_)[:n, :n]
        t = np.tril(t) if lower else np.triu(t)      # the triangle named
        if unit_diag:
            t = t - np.diag(np.diag(t)) + np.eye(n)
        assert np.isfinite(t).all()
        if side:
            b = self._view(dB, 0, ldb, r, np_)
            assert not b[:, n:].any()                # the pad is zero on entry
            # X op(T) = B  <=>  op(T)^T X^T = B^T
            b[:, :n] = scipy.linalg.solve_triangular(
                t, b[:, :n].T, lower=bool(lower), trans=0 if trans else 1).T
        else:
            b = self._view(dB, 0, ldb, np_, r)
            assert not b[n:, :].any()
            b[:n, :] = scipy.linalg.solve_triangular(
                t, b[:n, :], lower=bool(lower), trans=1 if trans else 0)
        return 0

    def map_raw(self, op, n, dA, dB, scalar, dC, fp32=False, check=True):
        assert op == "muls" and dB is None
        dC[:n] = dA[:n] * scalar
        return 0

    def gemm_grouped_raw(self, problems, fp32=False, accumulate=False,
                         trans_a=False, trans_b=False, check=True):
        for (m, k, n, bA, oA, lda, bB, oB, ldb, bC, oC, ldc) in problems:
            assert m % 128 == 0 and n % 128 == 0 and k % 16 == 0
            assert bC is not bA and bC is not bB
            a = (self._view(bA, oA, lda, k, m).T if trans_a
                 else self._view(bA, oA, lda, m, k))
            b = (self._view(bB, oB, ldb, n, k).T if trans_b
                 else self._view(bB, oB, ldb, k, n))
            c = self._view(bC, oC, ldc, m, n)
            assert np.isfinite(a).all() and np.isfinite(b).all()
            c[...] = (c if accumulate else 0) + a @ b
        return 0


def _spd(n, seed):
    r = gen_matrix(n, n, seed=seed)
    return (r + r.T) / 2 + n * np.eye(n)


@pytest.mark.parametrize("n,base", [(300, 128), (300, 96), (250, 64),
                                    (130, 128), (100, 128)])
def test_cholesky_trsm_panel_layout(n, base):
    eng = RawNumpyEngine()
    a = _spd(n, 2000 + n)
    L = DenseVecMatrix(a, engine=eng).choleskyDecompose(
        mode="dist", base_size=base, panel="trsm").toBreeze()
    assert np.allclose(np.triu(L, 1), 0)
    rel = np.max(np.abs(L @ L.T - a)) / np.max(np.abs(a))
    assert rel < 1e-12, rel
    nb = -(-n // base)
    # one right / lower / trans / non-unit solve per column panel
    assert len(eng.trsm_calls) == nb - 1
    assert all(c[2:] == (1, 1, 1, 0) for c in eng.trsm_calls)
    assert eng.live == 0                              # every buffer freed


def test_cholesky_panel_argument():
    a = _spd(60, 3000)
    with pytest.raises(ValueError):
        DenseVecMatrix(a, engine=RawNumpyEngine()).choleskyDecompose(
            mode="dist", base_size=32, panel="gemm")
    # the local route needs no engine whatever the panel
    L = DenseVecMatrix(a).choleskyDecompose(panel="trsm").toBreeze()
    assert np.max(np.abs(L @ L.T - a)) / np.max(np.abs(a)) < 1e-12


@pytest.mark.parametrize("cols", [None, 1, 3, 130])
def test_solve_local_factor_device_substitution(cols):
    n = 300
    eng = RawNumpyEngine()
    rng = np.random.RandomState(7)
    # rows shuffled, so that partial pivoting gives a p_array that is not
    # the identity and a wrong reading of it cannot pass
    a = (gen_matrix(n, n, seed=41) + n * np.eye(n))[rng.permutation(n), :]
    b = rng.uniform(-1, 1, size=n if cols is None else (n, cols))
    dvm = DenseVecMatrix(a, engine=eng)
    blocks, p_array = dvm.luDecompose(mode="local")
    assert (p_array != np.arange(n)).any()
    # the property the LU tests assert, which lu_solve's permutation reads
    lu = blocks.toBreeze()
    assert np.allclose(a[p_array, :],
                       (np.tril(lu, -1) + np.eye(n)) @ np.triu(lu))
    x = lu_solve(blocks, p_array, b)
    assert x.shape == b.shape
    ref = np.linalg.solve(a, b)
    assert np.max(np.abs(x - ref)) <= 1e-12 * np.max(np.abs(ref))
    np.testing.assert_array_equal(dvm.solve(b, mode="local"), x)
    # unit-lower first, then upper, on ONE uploaded factor
    assert [c[2:] for c in eng.trsm_calls[:2]] == [(0, 1, 0, 1), (0, 0, 0, 0)]
    assert eng.live == 0


def test_lu_solve_refuses_a_wrong_shape():
    eng = RawNumpyEngine()
    blocks, p = DenseVecMatrix(_spd(8, 1), engine=eng).luDecompose(mode="local")
    with pytest.raises(ValueError):
        lu_solve(blocks, p, np.zeros(7))
