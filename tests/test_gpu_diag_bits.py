# The two diagonal kernels (trsm_diag_kernel, getrf_diag_kernel) bit for
# bit on ROUNDING data. Both claim fixed arithmetic: one division and one
# fused multiply-add per element operation, in a fixed order
# (marlin_amd/csrc/getrf_plan.h, trsm_plan.h; include/marlin_gpu.h). On the
# exact data of test_gpu_trsm.py and test_gpu_getrf.py a multiplication by a
# reciprocal equals a division, a multiply and a subtract equal a fused
# multiply-add and any order of the updates gives the same bits, so those
# tests cannot tell. Here the data round at every operation and the device
# is compared with numpy restatements of the headers' arithmetic
# (_getrf_cases.eliminate_restated, _trsm_cases.substitute_restated, on the
# exact fma of tests/_fma.py), which test_diag_bits_cpu.py proves against
# the C++ on this same data and shows to differ from every degraded model.
#   1. GETRF, one block: standard-normal A with nothing dominant, so the
#      pivot search is decided by rounded values; image, piv, info.
#   2. GETRF in fp32 gradual underflow: A scaled by 2^-130.
#   3. GETRF, the NaN rule of the contract, and an inf tie.
#   4. GETRF, several blocks: the leading block, the two strip solves of
#      step 0 bit for bit, the rest under the residual bound (the trailing
#      matrix goes through the MFMA GEMM, whose bits are not restated).
#   5. TRSM, one block: all 16 forms.
# Every comparison is on bits after -0 -> +0, NaN matched as a class
# (_getrf_cases.same_bits).
import functools

import numpy as np
import pytest

import _getrf_cases as GC
import _trsm_cases as TC
from _exact import PAD, UINT, _nan, dtype_of
from marlin_amd import Engine

pytestmark = pytest.mark.gpu

W = 128
TYPES = pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])

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


def _same(got, want, what):
    bad = GC.same_bits(np.asarray(got), np.asarray(want))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} elements "
                           f"differ, first at (row, col) {bad[0]}")


# ---------------------------------------------------------------------------
# GETRF
def _factor(eng, fp32, a, what):
    """Runs the entry twice on a's poisoned image. Returns (info, the
    np x np image, piv[:np]) of the first run after the checks every case
    shares: the pitch pad still NaN, the guard entry of piv kept, piv the
    identity on the pad, the same bytes from the second run."""
    _require_healthy()
    dt = dtype_of(fp32)
    U = UINT[dt]
    n = a.shape[0]
    np_ = GC.r128(n)
    img = GC.a_image(a, np_ + PAD, dt)
    rc, info, outs, _ = GC.factor_image(eng, fp32, n, img, repeat=2)
    _rc_ok(rc, what)
    (got, piv), (again, piv2) = outs
    assert (got.view(U)[np_:, :] == _nan(dt).view(U)).all(), \
        f"{what}: the pitch pad was written"
    assert piv[np_] == -7, f"{what}: wrote past the np entries of dPiv"
    np.testing.assert_array_equal(piv[n:np_], np.arange(n, np_),
                                  err_msg=f"{what}: piv on the pad")
    np.testing.assert_array_equal(again.view(U), got.view(U),
                                  err_msg=f"{what}: second run differs")
    np.testing.assert_array_equal(piv2, piv)
    pad = np.ones((np_, np_), dtype=bool)
    pad[:n, :n] = False
    assert not got[:np_, :][pad].any(), f"{what}: a pad is not zero"
    return info, got[:np_, :], piv[:np_]


def _block(a, dt):
    blk = np.zeros((W, W), dtype=dt, order="F")
    blk[:a.shape[0], :a.shape[1]] = a
    return blk


@functools.lru_cache(maxsize=None)
def _restated_block(fp32, kind, n):
    """(A, (block after, perm, first_zero)) of a one-block problem, once."""
    a = {"normal": lambda: GC.normal_problem(fp32, n),
         "subnormal": lambda: GC.normal_problem(fp32, n, -130),
         "nan": lambda: GC.nan_problem(fp32)[0],
         "inf": lambda: GC.inf_problem(fp32)[0]}[kind]()
    return a, GC.eliminate_restated(_block(a, dtype_of(fp32)), n)


def _one_block(eng, fp32, kind, n):
    what = f"{'f32' if fp32 else 'f64'} {kind} n={n}"
    a, (want, perm, fz) = _restated_block(fp32, kind, n)
    assert fz == 0
    info, got, piv = _factor(eng, fp32, a, what)
    assert info == 0, what
    np.testing.assert_array_equal(piv, perm, err_msg=what)
    _same(got, want, what)
    return got, piv


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128])
@TYPES
def test_getrf_one_block_bits(eng, fp32, n):
    got, piv = _one_block(eng, fp32, "normal", n)
    assert np.isfinite(got).all()
    if n > 2:
        # nothing is dominant: rows did move, on rounded candidates
        assert (piv[:n] != np.arange(n)).sum() > n // 2


def test_getrf_fp32_gradual_underflow_bits(eng):
    a = GC.normal_problem(1, 128, -130)
    tiny = np.finfo(np.float32).tiny
    assert (np.abs(a) < tiny).all() and (a != 0).mean() > 0.9
    got, piv = _one_block(eng, 1, "subnormal", 128)
    u = np.triu(got)
    # nine tenths of U are subnormal and not flushed (element growth lifts
    # a few entries just past 2^-126), the multipliers are O(1)
    assert ((u != 0) & (np.abs(u) < tiny)).sum() > 0.9 * 128 * 129 / 2
    assert (np.abs(u) < 2.0 ** -120).all()
    assert (np.abs(np.tril(got, -1)) <= 1).all()


@TYPES
def test_getrf_nan_is_never_chosen_while_another_entry_remains(eng, fp32):
    a, r = GC.nan_problem(fp32)
    got, piv = _one_block(eng, fp32, "nan", 128)
    assert piv[127] == r, "the NaN row did not sink to the bottom"
    assert np.isfinite(got[:127, :]).all(), "another row met the NaN"
    assert np.isnan(got[127, :]).all()


@TYPES
def test_getrf_inf_tie_goes_to_the_lowest_row(eng, fp32):
    a, r1, r2 = GC.inf_problem(fp32)
    got, piv = _one_block(eng, fp32, "inf", 128)
    assert piv[0] == r1 and piv[127] == r2
    assert np.isinf(got[0, 0]) and np.isfinite(got[:127, 1:]).all()
    assert not got[1:127, 0].any() and np.isnan(got[127, :]).all()


@pytest.mark.parametrize("n", [129, 300])
@TYPES
def test_getrf_several_blocks_step0_bits(eng, fp32, n):
    dt = dtype_of(fp32)
    what = f"{'f32' if fp32 else 'f64'} n={n}"
    a = GC.normal_problem(fp32, n)
    np_ = GC.r128(n)
    img = np.zeros((np_, np_), dtype=dt, order="F")
    img[:n, :n] = a
    lu0, perm0, fz = GC.eliminate_restated(img[:W, :W], W)
    assert fz == 0
    info, got, piv = _factor(eng, fp32, a, what)
    assert info == 0 and np.isfinite(got).all(), what
    # (1) the leading block
    np.testing.assert_array_equal(piv[:W], perm0, err_msg=what)
    _same(got[:W, :W], lu0, f"{what}: block (0, 0)")
    # (4) U12 = L11^-1 (P A12): left / lower / unit on the permuted strip
    u12 = TC.substitute_restated((0, 1, 0, 1), lu0, img[perm0, W:], W)
    _same(got[:W, W:], u12, f"{what}: U12")
    # (3) L21 = A21 U11^-1: right / upper / non-unit; the later steps then
    # move its rows with their blocks' permutations
    l21 = TC.substitute_restated((1, 0, 0, 0), lu0, img[W:, :W], W)
    _same(got[W:, :W], l21[piv[W:] - W, :], f"{what}: L21")
    # the whole, through the MFMA GEMM: the residual bound
    ratio = GC.residual_ratio(fp32, a, got[:n, :n], piv[:n])
    print(f"getrf {what}: max residual / bound = {ratio:.4f}")
    assert ratio <= 1.0, f"{what}: residual is {ratio:.3f} x the bound"


# ---------------------------------------------------------------------------
# TRSM
@functools.lru_cache(maxsize=None)
def _restated_strip(fp32, form, n):
    timg, bimg = TC.block_images(fp32, form, n)
    tblk, strip = TC.block_of_images(form, timg, bimg)
    return timg, bimg, TC.substitute_restated(form, tblk, strip, n)


@pytest.mark.parametrize("form", TC.FORMS, ids=[TC.form_id(f) for f in TC.FORMS])
@TYPES
def test_trsm_one_block_bits(eng, fp32, form):
    dt = dtype_of(fp32)
    U = UINT[dt]
    side = form[0]
    r = 128
    for n in (1, 77, 128):
        _require_healthy()
        what = f"{'f32' if fp32 else 'f64'} {TC.form_id(form)} n={n}"
        timg, bimg, want = _restated_strip(fp32, form, n)
        rc, outs, _, tafter = TC.solve_images(eng, fp32, form, n, r, timg,
                                              bimg)
        _rc_ok(rc, what)
        got = outs[0][:r, :W] if side else outs[0][:W, :r]
        x, pad, sent = TC.split_b_image(outs[0], side, n, r)
        assert np.isfinite(x).all(), f"{what}: a NaN sentinel reached X"
        _same(got, want, what)
        assert (pad == 0).all(), f"{what}: B's pad [n, 128) is not zero"
        assert (outs[0].view(U)[sent] == _nan(dt).view(U)).all(), \
            f"{what}: B's pitch pad or guard column was written"
        assert (tafter.view(U) == timg.view(U)).all(), f"{what}: T was written"
