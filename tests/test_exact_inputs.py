# CPU-only checks of the exact-arithmetic GEMM test method (tests/_exact.py):
# the generated inputs respect the representability bounds the method
# relies on, the float64 reference is exact (pinned against an int64
# matmul), the expected-config restatement and the case tables are sane,
# and the method is sensitive where the old max-norm bar is not.
import numpy as np
import pytest

import _exact
from oracle import gen_matrix


def test_fp32_inputs_respect_bounds():
    # |entry| <= 15, integer; K <= 512 -> every partial sum (plus the
    # beta=1 seed) is an integer below 2^17 << 2^24
    c = _exact.Case(1, 1, 128, 128, _exact.F32_KMAX)
    a, b, c0, ref = _exact.gemm_inputs(c)
    for x in (a, b, c0):
        assert x.dtype == np.float32
        assert (x == np.rint(x)).all()
        assert np.abs(x).max() <= _exact.F32_AMAX
        # the full range is used and values vary along both axes
        assert x.min() == -_exact.F32_AMAX and x.max() == _exact.F32_AMAX
        assert (x[0, :] != x[1, :]).any() and (x[:, 0] != x[:, 1]).any()
    worst = _exact.F32_AMAX ** 2 * _exact.F32_KMAX + _exact.F32_AMAX
    assert worst < 2 ** 17 < 2 ** 24
    # worst-case |partial sum| in ANY order is bounded by sum |a||b| + |c0|
    bound = (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
             + np.abs(c0))
    assert bound.max() <= worst
    assert (ref == np.rint(ref)).all()
    assert (ref.astype(np.float32).astype(np.float64) == ref).all()


def test_fp64_inputs_respect_bounds():
    # entries q * 2^-19, |q| <= 2^19; K <= 4096 -> every partial sum is a
    # multiple of 2^-38 below 2^51 units: fits the 53-bit significand
    c = _exact.Case(0, 1, 128, 128, _exact.F64_KMAX)
    a, b, c0, ref = _exact.gemm_inputs(c)
    scale = 2.0 ** _exact.F64_QBITS
    for x in (a, b, c0):
        assert x.dtype == np.float64
        q = x * scale
        assert (q == np.rint(q)).all()
        assert np.abs(q).max() <= _exact.F64_QMAX
        assert np.abs(q).max() > _exact.F64_QMAX * 0.99
    worst_units = (_exact.F64_QMAX ** 2 * _exact.F64_KMAX
                   + _exact.F64_QMAX * 2 ** _exact.F64_QBITS)
    assert worst_units < 2 ** 51 < 2 ** 53
    units = ref * 2.0 ** (2 * _exact.F64_QBITS)
    assert (units == np.rint(units)).all()
    assert np.abs(units).max() < 2 ** 51


@pytest.mark.parametrize("fp32", [0, 1])
def test_float64_reference_is_exact_vs_int64(fp32):
    # smallest case of the table: the float64 matmul reference equals the
    # integer product exactly (int64 cannot overflow: |q1*q2|*K <= 2^43)
    c = _exact.Case(fp32, 1, 128, 128, 16)
    a, b, c0, ref = _exact.gemm_inputs(c)
    sa, sb, sc = _exact._seeds(c)
    _, qa = _exact.exact_matrix(c.M, c.K, sa, fp32)
    _, qb = _exact.exact_matrix(c.K, c.N, sb, fp32)
    _, qc = _exact.exact_matrix(c.M, c.N, sc, fp32)
    assert qa.dtype == qb.dtype == np.int64
    if fp32:
        exact = qa @ qb + qc
        np.testing.assert_array_equal(ref, exact.astype(np.float64))
    else:
        exact = qa @ qb + qc * (1 << _exact.F64_QBITS)     # units of 2^-38
        assert np.abs(exact).max() < 2 ** 53
        np.testing.assert_array_equal(
            ref, exact.astype(np.float64) * 2.0 ** (-2 * _exact.F64_QBITS))


def test_case_tables():
    cases = _exact.default_cases()
    assert len(cases) == len(set(cases)) == 36
    for c in cases + _exact.config_cases({"MARLIN_GEMM_CFG": "bk32"}) \
            + _exact.config_cases({"MARLIN_GEMM_CFG": "bm256"}):
        assert c.M % 128 == 0 and c.N % 128 == 0 and c.K % 16 == 0
        assert c.K <= _exact.F32_KMAX
    grids = {(c.M // 128, c.N // 128) for c in cases if c.K == 32}
    assert set(_exact.GRIDS) <= grids
    # every type x beta instantiation of the default geometry is present
    assert {(c.fp32, c.beta) for c in cases} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c.K // 16 for c in cases if c.M == 256} == {1, 2, 3, 5}


def test_expected_config_restates_the_launcher():
    C = _exact.Case
    e = _exact.expected_config
    base = {"is_fp32": 0, "beta_one": 0, "bk": 16, "bm": 128, "waves": 4,
            "band": 8, "phase_mask": 0}
    assert e({}, C(0, 0, 1152, 1152, 32)) == base
    assert e({}, C(0, 0, 384, 384, 32))["band"] == 3          # nbn < 8
    bk = {"MARLIN_GEMM_CFG": "bk32"}
    assert e(bk, C(1, 1, 256, 256, 64)) == dict(
        base, is_fp32=1, beta_one=1, bk=32, waves=8, band=2)
    assert e(bk, C(0, 0, 256, 256, 48))["bk"] == 16           # K % 32 != 0
    bm = {"MARLIN_GEMM_CFG": "bm256"}
    assert e(bm, C(0, 0, 2304, 1152, 32)) == dict(base, bm=256, waves=8)
    assert e(bm, C(0, 0, 384, 256, 32))["bm"] == 128          # M % 256 != 0
    assert e(bm, C(1, 0, 256, 256, 32))["bm"] == 128          # fp32 ignores bm
    assert e({"MARLIN_GEMM_REMAP": "bands"}, C(0, 0, 128, 2176, 32))["band"] == -8
    assert e({"MARLIN_GEMM_BAND": "16"}, C(0, 0, 128, 2176, 32))["band"] == 16
    assert e({"MARLIN_GEMM_BAND": "3"}, C(0, 0, 128, 128, 32))["band"] == 1
    assert e({"MARLIN_GEMM_PHASE": "8"}, C(0, 0, 128, 128, 32))["phase_mask"] == 8


def _old_bar(got, ref):
    # the measure every pre-existing GEMM test uses (rel_err in
    # test_gpu_parity.py): max|got-ref| / max|ref|, < 1e-4 for fp32
    return np.max(np.abs(got - ref)) / np.max(np.abs(ref))


def test_exact_method_catches_what_the_old_bar_passes():
    """Why the exact method exists: a kernel that drops ONE k-term.

    (1) Exact-integer fp32 case at K=512: the defective result fails
        assert_array_equal -- by at least 1 in every entry whose dropped
        product is non-zero.
    (2) The same defect under the old method -- uniform [0,1) fp32 inputs
        at the k=40000 working size of the long fp32 tests, where each C
        entry is ~k/4 -- moves the result by < 1e-4 of max|ref| and
        PASSES the old bar (measured below: ~9e-5 for the worst entry of
        this slice, ~2.5e-5 for a typical one).

    The old bar is only blind where C is large, i.e. at large k with
    all-positive inputs; at K=512 on the signed-integer data max|ref| is
    ~7e3 and one dropped term (up to 225) is ~3e-2 of it, so there the
    old bar would notice too. That figure is asserted as measured rather
    than claimed otherwise; the point of the exact method is that it is
    sensitive at the SMALL shapes that reach every kernel path, where
    the old tests never ran, and needs no bar at all."""
    c = _exact.Case(1, 0, 128, 128, _exact.F32_KMAX)
    a, b, _, ref = _exact.gemm_inputs(c)
    k0 = 257
    dropped = ref - np.outer(a[:, k0].astype(np.float64),
                             b[k0, :].astype(np.float64))
    got = dropped.astype(np.float32)              # still exact in fp32
    assert (got.astype(np.float64) == dropped).all()
    with pytest.raises(AssertionError):
        np.testing.assert_array_equal(got.astype(np.float64), ref)
    nbad = np.count_nonzero(got.astype(np.float64) != ref)
    assert nbad > 0.8 * ref.size                  # nearly every entry flags it
    assert _old_bar(got.astype(np.float64), ref) > 1e-4   # see docstring

    # (2) old method, old inputs, old working size: one slice of the
    # 40000^2 fp32 problem (128 rows x 8 cols of C, full k)
    k = 40000
    a_u = gen_matrix(128, k, seed=0xA11CE, dtype=np.float32)
    b_u = gen_matrix(k, 8, seed=0xB0B, dtype=np.float32)
    ref_u = a_u.astype(np.float64) @ b_u.astype(np.float64)
    k1 = 12345
    got_u = (ref_u - np.outer(a_u[:, k1].astype(np.float64),
                              b_u[k1, :].astype(np.float64))
             ).astype(np.float32).astype(np.float64)
    assert not (got_u == ref_u).all()
    assert _old_bar(got_u, ref_u) < 1e-4          # the defect passes
