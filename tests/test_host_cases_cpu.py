# CPU-only: the claims tests/_host_cases.py makes about its own tables,
# asserted from the generated data -- inputs inside the exactness bounds of
# _exact.py, the float64 reference equal to the int64 one, and the poison
# call's images at least as large as every image of every case.
import numpy as np
import pytest

import _exact
import _exact_summa as S
import _host_cases as H

ALL_SHAPES = sorted(set(H.SHAPES + H.SUMMA_SHAPES
                        + [s for _, s in H.NAMED.values()]))
FP = pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])


@FP
@pytest.mark.parametrize("m,k,n", ALL_SHAPES)
def test_inputs_inside_bounds_and_reference_is_int64(fp32, m, k, n):
    a, b, c0, add, q = H.gemm_inputs(fp32, m, k, n)
    qmax = _exact.F32_AMAX if fp32 else _exact.F64_QMAX
    assert k <= (_exact.F32_KMAX if fp32 else _exact.F64_KMAX)
    scale = 1.0 if fp32 else 2.0 ** -_exact.F64_QBITS
    for x, name in ((a, "a"), (b, "b"), (c0, "c0"), (add, "add")):
        assert x.dtype == _exact.dtype_of(fp32) and x.flags.f_contiguous
        assert np.abs(q[name]).max() <= qmax
        np.testing.assert_array_equal(x.astype(np.float64), q[name] * scale)
    f64 = lambda x: x.astype(np.float64)
    ref = f64(a) @ f64(b)
    # no rounding anywhere: the dtype holds the int64 result exactly
    np.testing.assert_array_equal(f64(H.expected(fp32, q)), ref)
    np.testing.assert_array_equal(f64(H.expected(fp32, q, q["c0"])),
                                  ref + f64(c0))
    assert np.abs(H.product_q(fp32, q, q["c0"])).max() < (
        2 ** 24 if fp32 else 2 ** 53)
    if fp32:                                   # the fused epilogue
        np.testing.assert_array_equal(f64(H.expected_t(q, False)), ref.T)
        np.testing.assert_array_equal(f64(H.expected_t(q, True)),
                                      ref.T + f64(add))


@FP
@pytest.mark.parametrize("m,k,n", H.SUMMA_SHAPES)
def test_summa_reference_is_int64(fp32, m, k, n):
    a, b, ref, qa, qb = S.summa_inputs(fp32, m, k, n)
    scale = 1.0 if fp32 else 2.0 ** (-2 * _exact.F64_QBITS)
    np.testing.assert_array_equal(ref, (qa @ qb) * scale)


@FP
@pytest.mark.parametrize("m,k,n", ALL_SHAPES)
def test_poison_covers_every_image(fp32, m, k, n):
    elem = 4 if fp32 else 8
    pa, pb, pc, padd = H.poison_bytes()
    ia, ib, ic = H.gemm_image_bytes(m, k, n, elem)
    assert ia <= pa and ib <= pb and ic <= pc
    if fp32:
        assert ic <= padd                      # add_c: as many elements as C
    # one-rank SUMMA host images: A mip x k, B roundup(k,16) x n (panel
    # loop), A mip x kp, B kp x njp (k-resident); C as above
    mip, njp, kp = H.roundup(m, 128), H.roundup(n, 128), H.roundup(k, 16)
    assert mip * k * elem <= pa and kp * n * elem <= pb
    assert mip * kp * elem <= pa and kp * njp * elem <= pb


def test_poison_operands_are_unpadded():
    m, k, n = H.POISON
    assert m % 128 == 0 and n % 128 == 0 and k % 16 == 0


def test_flat_cases_fit_under_the_poison_and_are_exact():
    pa, pb, pc, _ = H.poison_bytes()
    tm, tn = H.TRANSPOSE_SHAPE
    gm, gn = H.GEMV_SHAPE
    for elems in (H.MAP_N, H.SUM_N, tm * tn, gm * gn):
        assert elems * 8 < pa
    assert (gn + gm) * 8 < pb and 32 * gm * 8 < pc
    # every sum of products of the flat data is an integer below 2^53
    assert gn * H.FLAT_AMAX ** 2 < 2 ** 53 and H.SUM_N * H.FLAT_AMAX < 2 ** 53
    q = H.flat_ints(H.SUM_N, 1, 3)
    assert np.abs(q).max() <= H.FLAT_AMAX and q.dtype == np.int64
