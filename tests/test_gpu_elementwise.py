# GPU parity for the elementwise/scalar op family — the reference's own
# golden literals (DistributedMatrixSuite.scala:164-205 "element-wise
# addition/subtract ...", :319-324 "sum", :326-338 "dot product",
# :302-316 transpose), restated as data, run through the engine's
# mx_map/mx_sum/mx_transpose via the operator mirror.
import ctypes
import math

import numpy as np
import pytest

from marlin_amd import Engine, DenseVecMatrix
from marlin_amd import engine as E
from oracle import gen_matrix

pytestmark = pytest.mark.gpu

M4 = np.array([[0., 1, 2, 3], [2, 3, 4, 5], [3, 2, 1, 0], [1, 1, 1, 1]])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def dvm(eng):
    return DenseVecMatrix(M4, engine=eng)


def blk(eng):
    return DenseVecMatrix(M4, engine=eng).toBlockMatrix(2, 2)


def test_elementwise_golden(eng):
    ele_add1 = M4 + 1
    add_self = M4 + M4
    ele_sub1 = M4 - 1
    divide2 = M4 / 2
    for mat in (dvm(eng), blk(eng)):
        np.testing.assert_array_equal(mat.add(1).toBreeze(), ele_add1)
        np.testing.assert_array_equal(mat.add(mat).toBreeze(), add_self)
        np.testing.assert_array_equal(mat.subtract(1).toBreeze(), ele_sub1)
        np.testing.assert_array_equal(mat.subtract(mat).toBreeze(),
                                      np.zeros((4, 4)))
        np.testing.assert_array_equal(mat.multiply(2).toBreeze(), add_self)
        np.testing.assert_array_equal(mat.divide(2).toBreeze(), divide2)
    # cross-type: BlockMatrix op DenseVecMatrix
    np.testing.assert_array_equal(blk(eng).add(dvm(eng)).toBreeze(), add_self)
    np.testing.assert_array_equal(blk(eng).subtract(dvm(eng)).toBreeze(),
                                  np.zeros((4, 4)))


def test_subtract_by_divide_by(eng):
    np.testing.assert_array_equal(dvm(eng).subtractBy(10).toBreeze(), 10 - M4)
    m = M4 + 1
    got = DenseVecMatrix(m, engine=eng).divideBy(2).toBreeze()
    np.testing.assert_array_equal(got, 2 / m)


def test_sum_golden(eng):
    # DistributedMatrixSuite.scala:319-324: sum == 30.0
    assert dvm(eng).sum() == 30.0
    assert blk(eng).sum() == 30.0


def test_dot_product_golden(eng):
    # DistributedMatrixSuite.scala:326-338 ("dot product" = elementwise mul)
    expected = M4 * M4
    np.testing.assert_array_equal(dvm(eng).dotProduct(dvm(eng)).toBreeze(),
                                  expected)
    np.testing.assert_array_equal(blk(eng).dotProduct(blk(eng)).toBreeze(),
                                  expected)
    np.testing.assert_array_equal(dvm(eng).dotProduct(blk(eng)).toBreeze(),
                                  expected)


def test_transpose(eng):
    # DistributedMatrixSuite.scala:302-316
    np.testing.assert_array_equal(dvm(eng).transpose().toBreeze(), M4.T)
    np.testing.assert_array_equal(blk(eng).transpose().toBreeze(), M4.T)
    # ragged + larger
    a = gen_matrix(517, 301, seed=99)
    got = DenseVecMatrix(a, engine=eng).transpose().toBreeze()
    np.testing.assert_array_equal(got, a.T)


def test_elementwise_large_random(eng):
    a = gen_matrix(1000, 700, seed=1)
    b = gen_matrix(1000, 700, seed=2)
    e = eng
    np.testing.assert_array_equal(e.map_op("add", a, b), a + b)
    np.testing.assert_array_equal(e.map_op("sub", a, b), a - b)
    np.testing.assert_array_equal(e.map_op("emul", a, b), a * b)
    np.testing.assert_array_equal(e.map_op("muls", a, scalar=3.5), a * 3.5)
    np.testing.assert_array_equal(e.map_op("rdivs", a, scalar=1.0), 1.0 / a)
    assert abs(e.sum(a) - a.sum()) / abs(a.sum()) < 1e-12


def test_dimension_mismatch(eng):
    with pytest.raises(ValueError):
        dvm(eng).add(DenseVecMatrix(np.ones((3, 4)), engine=eng))


# ---------------------------------------------------------------------------
# fp32 instantiations of map/sum/transpose (the engine wrappers always
# pass is_fp32=0, so these go through the C ABI directly) and the scalar
# ops at a size where the grid-stride loops run: 1000x700 = 700000
# elements > the 2048x256 = 524288-thread map grid and the 1024x256 =
# 262144-thread sum grid.
BIG = (1000, 700)


def _vp(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _map32(eng, op, a, b=None, scalar=0.0):
    c = np.empty_like(a)
    rc = E.lib().mx_map(eng._ctx, Engine.OPS[op], 1, a.size, _vp(a),
                        _vp(b) if b is not None else None, float(scalar),
                        _vp(c))
    assert rc == 0, rc
    return c


def test_map_fp32_all_ops_bitexact(eng):
    # inputs in [0.5, 1.5): bounded away from 0 for rdivs, no subnormal
    # results. Every op is ONE IEEE-754 binary32 operation on the scalar
    # cast to float32 first (as map_kernel does), so numpy's float32
    # result is the exact expectation.
    a = gen_matrix(*BIG, seed=11, dtype=np.float32) + np.float32(0.5)
    b = gen_matrix(*BIG, seed=12, dtype=np.float32) + np.float32(0.5)
    assert a.dtype == np.float32 and a.min() >= 0.5
    s64 = 3.3                        # not representable in float32
    s = np.float32(s64)
    expect = {
        "add": a + b, "sub": a - b, "emul": a * b,
        "adds": a + s, "subs": a - s, "rsubs": s - a,
        "muls": a * s, "divs": a / s, "rdivs": s / a,
    }
    assert set(expect) == set(Engine.OPS)
    for op, ref in expect.items():
        assert ref.dtype == np.float32
        got = _map32(eng, op, a, b if Engine.OPS[op] <= 2 else None, s64)
        np.testing.assert_array_equal(got.view(np.uint32),
                                      ref.view(np.uint32), err_msg=op)


def test_map_fp64_scalar_ops_large(eng):
    # adds/subs/rsubs/divs were only ever checked on a 4x4 matrix
    a = gen_matrix(*BIG, seed=13) + 0.5
    s = 3.3
    np.testing.assert_array_equal(eng.map_op("adds", a, scalar=s), a + s)
    np.testing.assert_array_equal(eng.map_op("subs", a, scalar=s), a - s)
    np.testing.assert_array_equal(eng.map_op("rsubs", a, scalar=s), s - a)
    np.testing.assert_array_equal(eng.map_op("divs", a, scalar=s), a / s)


def test_sum_fp32_accumulates_in_double(eng):
    # sum_stage1_kernel<float> widens each element to double (exact) and
    # adds in double; stage 2 adds the partials in double. Any summation
    # order of n terms with unit roundoff u = 2^-53 obeys
    #   |fl(sum) - sum| <= gamma_{n-1} * sum|a_i|,
    #   gamma_{n-1} = (n-1)u / (1 - (n-1)u) <= n*u   (as n(n-1)u <= 1),
    # so the bound is n * 2^-53 * sum|a|, against the correctly rounded
    # math.fsum of the same float32 values. Mixed signs make sum|a| the
    # honest scale (the sum itself nearly cancels).
    a = gen_matrix(*BIG, seed=14, dtype=np.float32) - np.float32(0.5)
    n = a.size
    assert n * (n - 1) * 2.0 ** -53 <= 1
    out = ctypes.c_double()
    rc = E.lib().mx_sum(eng._ctx, 1, n, _vp(a), ctypes.byref(out))
    assert rc == 0, rc
    vals = a.ravel(order="F").astype(np.float64)
    exact = math.fsum(vals.tolist())
    bound = n * 2.0 ** -53 * math.fsum(np.abs(vals).tolist())
    assert abs(out.value - exact) <= bound, (out.value, exact, bound)


@pytest.mark.parametrize("shape", [(517, 301), (33, 1)])
def test_transpose_fp32(eng, shape):
    m, n = shape
    a = gen_matrix(m, n, seed=15, dtype=np.float32)
    c = np.full((n, m), np.nan, dtype=np.float32, order="F")
    rc = E.lib().mx_transpose(eng._ctx, 1, m, n, _vp(a), _vp(c))
    assert rc == 0, rc
    np.testing.assert_array_equal(c, a.T)
