# The device LU factorisation (mx_getrf_device): a blocked right-looking
# sweep of the diagonal kernel, the row-permutation kernel, two strip solves
# and one accumulating GEMM per step (include/marlin_gpu.h has the
# contract).
#   1. exact data (tests/_getrf_cases.py, proven on the CPU by
#      test_getrf_cases.py) in both types at orders around the block edge:
#      packed L\U, the pads, the permutation and info bit for bit, NaN in
#      the pitch pad, the same bytes from a second run;
#   2. a tie (the lowest row wins) and a zero pivot (info, the sweep
#      finishes, lu_factor_device raises);
#   3. rounding data against the componentwise backward-error bound of
#      Gaussian elimination;
#   4. refusals touch nothing; the empty call.
import ctypes

import numpy as np
import pytest

import _getrf_cases as GC
from _exact import PAD, UINT, _dev, _filled, _nan, dtype_of
from marlin_amd import DenseVecMatrix, Engine
from marlin_amd.engine import lib
from marlin_amd.linalg import lu_factor_device

pytestmark = pytest.mark.gpu

EINVAL = GC.EINVAL
Z = GC.zero_sign_dropped

# Once a call of this module has come back with a HIP failure nothing
# further is started on the device: every remaining test fails immediately
# with the first failure's reason.
_GPU_POISONED = []


def _require_healthy():
    if _GPU_POISONED:
        pytest.fail("not run: an earlier GPU call of this module failed "
                    f"hard ({_GPU_POISONED[0]})", pytrace=False)


def _rc_ok(rc, what):
    if rc == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure")
    assert rc == 0, f"{what}: entry returned {rc}"


@pytest.fixture(scope="module")
def eng():
    _require_healthy()
    e = Engine(0)
    yield e
    e.close()


def _factor(eng, fp32, a, what, repeat=1, pad=PAD):
    """Runs the entry on a's poisoned image; returns (info, image, piv,
    stats) of the first run after the checks every case shares: the pitch
    pad and the guard entry untouched, the pads of piv the identity, and
    (repeat = 2) the same bytes from a second run on a fresh upload."""
    _require_healthy()
    dt = dtype_of(fp32)
    U = UINT[dt]
    n = a.shape[0]
    np_ = GC.r128(n)
    img = GC.a_image(a.astype(dt), np_ + pad, dt)
    rc, info, outs, st = GC.factor_image(eng, fp32, n, img, repeat)
    _rc_ok(rc, what)
    got, piv = outs[0]
    if pad:
        assert (got.view(U)[np_:, :] == _nan(dt).view(U)).all(), \
            f"{what}: the pitch pad was written"
    assert piv[np_] == -7, f"{what}: wrote past the np entries of dPiv"
    np.testing.assert_array_equal(piv[n:np_], np.arange(n, np_),
                                  err_msg=f"{what}: piv on the pad")
    for again, piv2 in outs[1:]:
        np.testing.assert_array_equal(again.view(U), got.view(U),
                                      err_msg=f"{what}: second run differs")
        np.testing.assert_array_equal(piv2, piv)
    assert st["flops"] == 2.0 * n * n * n / 3.0
    assert st["gemm_launches"] == np_ // 128 - 1
    return info, got[:np_, :], piv[:n], st


def _padded(packed, dt):
    n = packed.shape[0]
    np_ = GC.r128(n)
    want = np.zeros((np_, np_), dtype=dt, order="F")
    want[:n, :n] = packed
    return want


# ---------------------------------------------------------------------------
# 1. exact
@pytest.mark.parametrize("n", GC.ORDERS)
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_getrf_exact(eng, fp32, n):
    dt = dtype_of(fp32)
    U = UINT[dt]
    what = f"{'f32' if fp32 else 'f64'} n={n}"
    a, packed, p = GC.exact_problem(n)
    info, got, piv, _ = _factor(eng, fp32, a, what, repeat=2)
    assert info == 0, what
    np.testing.assert_array_equal(piv, p, err_msg=what)
    # bits, after -0 -> +0 and nothing else (_getrf_cases.zero_sign_dropped)
    bad = np.argwhere(Z(got).view(U) != _padded(packed, dt).view(U))
    assert len(bad) == 0, f"{what}: first mismatch at (row, col) {bad[0]}"
    pad = np.ones(got.shape, dtype=bool)
    pad[:n, :n] = False
    assert not got[pad].any(), f"{what}: a pad is not zero"


# ---------------------------------------------------------------------------
# 2. a tie; a zero pivot
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_getrf_tie_goes_to_the_lowest_row(eng, fp32):
    dt = dtype_of(fp32)
    U = UINT[dt]
    a, packed, p = GC.tie_problem()
    want_lu, want_piv, want_info = GC.block_lu(a.astype(dt))
    info, got, piv, _ = _factor(eng, fp32, a, "tie", repeat=2)
    assert info == want_info == 0
    np.testing.assert_array_equal(piv, want_piv)
    np.testing.assert_array_equal(Z(got).view(U),
                                  Z(_padded(want_lu, dt)).view(U))


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_getrf_zero_pivot_is_reported_and_the_sweep_finishes(eng, fp32):
    dt = dtype_of(fp32)
    U = UINT[dt]
    a, _, _ = GC.zero_pivot_problem()
    j = GC.ZERO_COL - 1
    want_lu, want_piv, want_info = GC.block_lu(a.astype(dt))
    assert want_info == GC.ZERO_COL
    info, got, piv, _ = _factor(eng, fp32, a, "zero pivot")   # rc == MX_OK
    assert info == GC.ZERO_COL
    np.testing.assert_array_equal(piv, want_piv)
    n = a.shape[0]
    # the columns before it, in every row; and the whole of its own block,
    # which went on to the end with the column left unscaled
    np.testing.assert_array_equal(Z(got[:n, :j]).view(U),
                                  Z(want_lu[:, :j]).view(U))
    np.testing.assert_array_equal(Z(got[:128, :128]).view(U),
                                  Z(want_lu[:128, :128]).view(U))
    assert got[j, j] == 0


def test_lu_factor_device_raises_on_a_zero_pivot(eng):
    _require_healthy()
    a, _, _ = GC.zero_pivot_problem()
    with pytest.raises(np.linalg.LinAlgError, match=f"column {GC.ZERO_COL}"):
        lu_factor_device(DenseVecMatrix(np.array(a), engine=eng))


# ---------------------------------------------------------------------------
# 3. rounding data
@pytest.mark.parametrize("shuffled", [False, True],
                         ids=["dominant", "rows-shuffled"])
@pytest.mark.parametrize("n", [129, 300])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_getrf_componentwise_residual(eng, fp32, n, shuffled):
    what = (f"{'f32' if fp32 else 'f64'} n={n} "
            f"{'rows-shuffled' if shuffled else 'dominant'}")
    a, src = GC.rounding_problem(fp32, n, shuffled)
    info, got, piv, _ = _factor(eng, fp32, a, what, repeat=2, pad=0)
    assert info == 0 and np.isfinite(got).all(), what
    # the dominant diagonal is the pivot: the shuffle is undone
    np.testing.assert_array_equal(src[piv], np.arange(n), err_msg=what)
    ratio = GC.residual_ratio(fp32, a, got[:n, :n], piv)
    print(f"getrf {what}: max residual / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: residual is {ratio:.3f} x the bound"
    assert not got[n:, :].any() and not got[:, n:].any(), what


# ---------------------------------------------------------------------------
# 4. refusals and the empty call
def test_getrf_refusals_touch_nothing(eng):
    _require_healthy()
    dt, U = np.float64, np.uint64
    n, np_ = 129, 256
    lda = np_ + PAD
    # the image exactly as large as the neighbouring legal call needs
    img = _filled(lda, np_, _nan(dt)).ravel(order="F")[:(np_ - 1) * lda + np_]
    img = np.ascontiguousarray(img)
    piv0 = np.full(np_, -7, dtype=np.int32)
    wide = _filled(lda + 2, np_, _nan(dt))        # room for a pitch of lda + 1
    bufs = []
    try:
        dA, dP, dW = _dev(eng, img, bufs), _dev(eng, piv0, bufs), \
            _dev(eng, wide, bufs)
        dA_short = eng.alloc(img.nbytes - 1)      # the image one byte too large
        bufs.append(dA_short)
        dP_short = eng.alloc(piv0.nbytes - 1)
        bufs.append(dP_short)

        def call(fp32=0, n=n, A=dA, lda=lda, P=dP):
            rc, info = eng.getrf_raw(n, A, lda, P, fp32, check=False)
            assert (info is None) == (rc != 0)
            return rc
        refused = {
            "is_fp32 = 2": dict(fp32=2),
            "is_fp32 = -1": dict(fp32=-1),
            "n = -1": dict(n=-1),
            "n one block past the image and dPiv": dict(n=2 * 128 + 1),
            "lda below np": dict(lda=np_ - 2),
            "lda not a multiple of 16 bytes": dict(A=dW, lda=lda + 1),
            "lda two elements past its buffer": dict(lda=lda + 2),
            "image one byte too large for its buffer": dict(A=dA_short),
            "dPiv one byte short": dict(P=dP_short),
            "dPiv == dA": dict(P=dA),
            "dA == dPiv": dict(A=dP),
            "dA NULL": dict(A=None),
            "dPiv NULL": dict(P=None),
        }
        for what, kw in refused.items():
            assert call(**kw) == EINVAL, what
            st = eng.stats()
            assert st["gemm_launches"] == 0 and st["gemm_ms"] == 0, what
        # a NULL info
        assert lib().mx_getrf_device(eng._ctx, 0, n, dA, lda, dP, None) == EINVAL
        assert lib().mx_getrf_device(eng._ctx, 0, 0, dA, lda, dP, None) == EINVAL
        np.testing.assert_array_equal(GC.fetch(eng, dA, img).view(U),
                                      img.view(U))
        np.testing.assert_array_equal(GC.fetch(eng, dP, piv0), piv0)
        np.testing.assert_array_equal(GC.fetch(eng, dW, wide).view(U),
                                      wide.view(U))
        # the empty call: MX_OK, info 0, nothing touched or looked at
        info = ctypes.c_int(-1)
        assert lib().mx_getrf_device(eng._ctx, 0, 0, None, 0, None,
                                     ctypes.byref(info)) == 0
        assert info.value == 0
        assert eng.getrf_raw(0, dA, lda, dP) == (0, 0)
        assert eng.stats()["gemm_launches"] == 0
        assert call(n=0, fp32=2) == EINVAL        # the flag still counts
        np.testing.assert_array_equal(GC.fetch(eng, dA, img).view(U),
                                      img.view(U))
        np.testing.assert_array_equal(GC.fetch(eng, dP, piv0), piv0)
    finally:
        for d in bufs:
            eng.free(d)
    # the call they all neighbour passes, at exactly this pitch and size
    a, packed, p = GC.exact_problem(n)
    full = GC.a_image(a, lda, dt)
    tight = np.ascontiguousarray(full.ravel(order="F")[:(np_ - 1) * lda + np_])
    bufs = []
    try:
        dA = _dev(eng, tight, bufs)
        dP = eng.alloc(np_ * 4)
        bufs.append(dP)
        rc, info = eng.getrf_raw(n, dA, lda, dP, check=False)
        _rc_ok(rc, "the neighbouring legal call")
        got = GC.fetch(eng, dA, tight)
        piv = np.empty(np_, dtype=np.int32)
        eng.download(piv, dP, piv.nbytes)
    finally:
        for d in bufs:
            eng.free(d)
    assert info == 0
    np.testing.assert_array_equal(piv[:n], p)
    back = np.full(lda * np_, np.nan)
    back[:tight.size] = got
    back = back.reshape((lda, np_), order="F")
    np.testing.assert_array_equal(Z(back[:n, :n]).view(U), packed.view(U))
