# The device triangular solve (mx_trsm_device): a blocked sweep of diagonal
# kernels and accumulating GEMMs (include/marlin_gpu.h has the contract).
#   1. exact data (tests/_trsm_cases.py) for all 16 forms, both types,
#      orders around the block edge and two right-hand-side counts: X bit
#      for bit, with NaN in everything that must not be read or written;
#   2. rounding data against the componentwise backward-error bound of
#      substitution, and the same bits from a second run;
#   3. refusals touch no buffer; empty shapes;
#   4. one packed L\U buffer read as unit-lower, then as upper;
#   5. the workspace across calls of growing and shrinking size.
import numpy as np
import pytest

import _exact
import _trsm_cases as TC
from _exact import PAD, UINT, _dev, _filled, _nan, dtype_of
from marlin_amd import Engine

pytestmark = pytest.mark.gpu

EINVAL = TC.EINVAL

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


def _what(fp32, form, n, r):
    return f"{'f32' if fp32 else 'f64'} {TC.form_id(form)} n={n} r={r}"


# ---------------------------------------------------------------------------
# 1. exact
@pytest.mark.parametrize("form", TC.FORMS, ids=[TC.form_id(f) for f in TC.FORMS])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_trsm_exact(eng, fp32, form):
    for n in TC.ORDERS:
        for r in TC.RHS:
            _require_healthy()
            what = _what(fp32, form, n, r)
            rec = TC.run_exact(eng, fp32, form, n, r)
            _rc_ok(rec["rc"], what)
            assert rec["finite"], f"{what}: a NaN sentinel reached the result"
            assert rec["first_bad"] is None, \
                f"{what}: first mismatch at (row, col) {rec['first_bad']}"
            assert rec["pad_zero"], f"{what}: B's pad [n, np) is not zero"
            assert rec["sentinels_kept"], \
                f"{what}: B's pitch pad or guard column was written"
            assert rec["t_untouched"], f"{what}: T was written"
            assert rec["flops"] == float(n) * n * r
            assert rec["launches"] == TC.r128(n) // 128 - 1


# ---------------------------------------------------------------------------
# 2. rounding data
ROUNDING = [(side, lower, trans, 0) for side in (0, 1) for lower in (0, 1)
            for trans in (0, 1)]


@pytest.mark.parametrize("n", [129, 300])
@pytest.mark.parametrize("form", ROUNDING,
                         ids=[TC.form_id(f) for f in ROUNDING])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_trsm_backward_error_and_repeatability(eng, fp32, form, n):
    _require_healthy()
    side, lower, trans, unit = form
    r = 128
    dt = dtype_of(fp32)
    what = _what(fp32, form, n, r)
    t, b = TC.rounding_problem(fp32, side, lower, trans, n, r)
    np_ = TC.r128(n)
    timg = TC.t_image(t, lower, unit, np_, dt)
    bimg = TC.b_image(b, side, n, r, r if side else np_, dt)
    rc, outs, _, _ = TC.solve_images(eng, fp32, form, n, r, timg, bimg,
                                     repeat=2)
    _rc_ok(rc, what)
    x = TC.split_b_image(outs[0], side, n, r)[0]
    assert np.isfinite(x).all(), what
    ratio = TC.residual_ratio(fp32, form, t, b, x)
    print(f"{what}: max residual / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: residual is {ratio:.3f} x the bound"
    U = UINT[dt]
    np.testing.assert_array_equal(outs[0].view(U), outs[1].view(U),
                                  err_msg=f"{what}: second run differs")


# ---------------------------------------------------------------------------
# 3. refusals and empty shapes
@pytest.mark.parametrize("side", [0, 1], ids=["left", "right"])
def test_trsm_refusals_touch_nothing(eng, side):
    _require_healthy()
    dt, U = np.float64, np.uint64
    n, r = 129, 128
    np_ = 256
    nan = _nan(dt)
    # both images exactly as large as the neighbouring legal call needs
    ldt, ldb = np_ + PAD, (r if side else np_) + PAD
    timg = _filled(ldt, np_, nan)
    bcols = np_ if side else r
    bimg = _filled(ldb, bcols, nan)
    small = _filled(128, 128, nan)            # a buffer too small for either
    bufs = []
    try:
        dT, dB = _dev(eng, timg, bufs), _dev(eng, bimg, bufs)
        dS = _dev(eng, small, bufs)

        def call(fp32=0, side=side, lower=1, trans=0, unit=0, n=n, r=r, T=dT,
                 ldt=ldt, B=dB, ldb=ldb):
            return eng.trsm_raw(n, r, T, ldt, B, ldb, side, lower, trans, unit,
                                fp32, check=False)
        refused = {
            "is_fp32 = 2": dict(fp32=2),
            "side = 2": dict(side=2),
            "side = -1": dict(side=-1),
            "lower = 2": dict(lower=2),
            "trans = 2": dict(trans=2),
            "unit_diag = -1": dict(unit=-1),
            "n = -1": dict(n=-1),
            "r = -128": dict(r=-128),
            "r not a multiple of 128": dict(r=r - 1),
            "r one block past B": dict(r=r + 128),
            "n one block past T and B": dict(n=2 * 128 + 1),
            "ldt below np": dict(ldt=np_ - 2),
            "ldt not a multiple of 16 bytes": dict(ldt=ldt + 1),
            "ldt two elements past its buffer": dict(ldt=ldt + 2),
            "ldb below its rows": dict(ldb=(r if side else np_) - 2),
            "ldb not a multiple of 16 bytes": dict(ldb=ldb + 1),
            "ldb two elements past its buffer": dict(ldb=ldb + 2),
            "T too small": dict(T=dS),
            "B too small": dict(B=dS),
            "dB == dT": dict(B=dT, ldb=ldt),
            "dT == dB": dict(T=dB, ldt=ldb),
            "dT NULL": dict(T=None),
            "dB NULL": dict(B=None),
        }
        for what, kw in refused.items():
            assert call(**kw) == EINVAL, what
            st = eng.stats()
            assert st["gemm_launches"] == 0 and st["gemm_ms"] == 0, what
        for d, img in ((dT, timg), (dB, bimg), (dS, small)):
            np.testing.assert_array_equal(TC.fetch(eng, d, img).view(U),
                                          img.view(U))
        # empty shapes: MX_OK, nothing touched, not even looked at
        assert call(n=0) == 0 and call(r=0) == 0 and call(n=0, r=0) == 0
        assert call(n=0, T=None, B=None, ldt=0, ldb=0) == 0
        assert eng.stats()["gemm_launches"] == 0
        assert call(n=0, side=2) == EINVAL      # the flags still count
        for d, img in ((dT, timg), (dB, bimg)):
            np.testing.assert_array_equal(TC.fetch(eng, d, img).view(U),
                                          img.view(U))
    finally:
        for d in bufs:
            eng.free(d)
    # the call they all neighbour passes, at exactly these pitches
    form = (side, 1, 0, 0)
    t, x, b = TC.exact_problem(side, 1, 0, 0, n, r)
    bim = TC.b_image(b, side, n, r, ldb, dt)[:, :bcols]
    rc, outs, _, _ = TC.solve_images(eng, 0, form, n, r,
                                     TC.t_image(t, 1, 0, ldt, dt),
                                     np.asfortranarray(bim))
    _rc_ok(rc, "the neighbouring legal call")
    np.testing.assert_array_equal(
        TC.zero_sign_dropped(TC.split_b_image(outs[0], side, n, r)[0]).view(U),
        TC.zero_sign_dropped(x).view(U))


# ---------------------------------------------------------------------------
# 4. packed L\U: the solve pattern
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [129, 300])
def test_trsm_packed_lu_one_buffer(eng, fp32, n):
    _require_healthy()
    dt = dtype_of(fp32)
    r = 128
    tl, _, _ = TC.exact_problem(0, 1, 0, 1, n, r)      # unit lower
    tu, x, bu = TC.exact_problem(0, 0, 0, 0, n, r)     # upper: U x = bu
    packed = np.tril(tl, -1) + tu                      # L\U, L's diagonal implied
    b = tl @ bu                                        # L (U x) = b, exact
    np_ = TC.r128(n)
    # every element of the packed image is referenced by one of the two
    # reads: no poison inside, zero pads as upload_matrix leaves them
    timg = np.zeros((np_, np_), dtype=dt, order="F")
    timg[:n, :n] = packed
    bimg = TC.b_image(b.astype(dt), 0, n, r, np_ + PAD, dt)
    bufs = []
    try:
        dT, dB = _dev(eng, timg, bufs), _dev(eng, bimg, bufs)
        _rc_ok(eng.trsm_raw(n, r, dT, np_, dB, np_ + PAD, 0, 1, 0, 1, fp32,
                            check=False), "L")
        mid = TC.fetch(eng, dB, bimg)
        _rc_ok(eng.trsm_raw(n, r, dT, np_, dB, np_ + PAD, 0, 0, 0, 0, fp32,
                            check=False), "U")
        got = TC.fetch(eng, dB, bimg)
    finally:
        for d in bufs:
            eng.free(d)
    U = UINT[dt]
    # bit for bit once -0 is written +0: the sign of an exact zero is not
    # X's (_trsm_cases.py); nothing else is normalised
    Z = TC.zero_sign_dropped
    np.testing.assert_array_equal(Z(mid[:n, :r]).view(U),
                                  Z(bu.astype(dt)).view(U))
    np.testing.assert_array_equal(Z(got[:n, :r]).view(U),
                                  Z(x.astype(dt)).view(U))
    assert not got[n:np_, :r].any()
    sent = TC.split_b_image(got, 0, n, r)[2]
    assert (got.view(U)[sent] == _nan(dt).view(U)).all()


# ---------------------------------------------------------------------------
# 5. the workspace
def test_trsm_workspace_across_calls():
    _require_healthy()
    form, n = (0, 1, 0, 0), 300
    sizes = [128, 512, 256, 128]

    def run(e, r):
        t, b = TC.rounding_problem(0, 0, 1, 0, n, r)
        rc, outs, _, _ = TC.solve_images(
            e, 0, form, n, r, TC.t_image(t, 1, 0, 384, np.float64),
            TC.b_image(b, 0, n, r, 384, np.float64))
        _rc_ok(rc, f"r={r}")
        return outs[0].view(np.uint64)

    one = Engine(0)
    try:
        grown = [run(one, r) for r in sizes]
    finally:
        one.close()
    for r, got in zip(sizes, grown):
        _require_healthy()
        fresh = Engine(0)
        try:
            np.testing.assert_array_equal(got, run(fresh, r),
                                          err_msg=f"r={r}")
        finally:
            fresh.close()
