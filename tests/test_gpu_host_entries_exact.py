# Exact GPU tests of the host-buffer entries on a dirtied workspace: every
# case runs right after a call that left NaN in each workspace it stages
# into (tests/_host_cases.py says why and test_host_cases_cpu.py checks the
# sizes), on exact inputs, and is compared with the int64 product by
# assert_array_equal. There is no tolerance in this module.
import ctypes

import numpy as np
import pytest

import _exact_summa as S
import _host_cases as H
from _exact import dtype_of
from marlin_amd import Engine
from marlin_amd import engine as E

pytestmark = pytest.mark.gpu

ENOMEM = -3
FP = pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
SHAPE = pytest.mark.parametrize("m,k,n", H.SHAPES)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.comm_init(0, 1, Engine.comm_id())     # the one-rank SUMMA entries
    yield e
    e.close()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got, want)


@FP
@SHAPE
@pytest.mark.parametrize("ta,tb", H.FORMS, ids=["nn", "tn", "nt", "tt"])
def test_gemm_op_after_poison(eng, fp32, m, k, n, ta, tb):
    a, b, _, _, q = H.gemm_inputs(fp32, m, k, n)
    H.poison(eng)
    gemm = eng.sgemm if fp32 else eng.dgemm
    got = gemm(H.stored(a, ta), H.stored(b, tb), trans_a=ta, trans_b=tb)
    _same(got, H.expected(fp32, q))


@pytest.mark.parametrize("name", sorted(H.NAMED))
def test_plain_entry_by_name_after_poison(eng, name):
    fp32, (m, k, n) = H.NAMED[name]
    dt = dtype_of(fp32)
    a, b, _, _, q = H.gemm_inputs(fp32, m, k, n)
    got = np.full((m, n), np.nan, dtype=dt, order="F")
    H.poison(eng)
    rc = getattr(E.lib(), name)(eng._ctx, m, k, n, E._fbuf(a, dt),
                                E._fbuf(b, dt), E._fbuf(got, dt))
    assert rc == 0
    _same(got, H.expected(fp32, q))


@SHAPE
def test_tile_dgemm_acc_after_poison(eng, m, k, n):
    """beta = 1: the seed goes through the same stage-in as A and B; its
    pad must be zero and the seed must arrive intact."""
    a, b, c0, _, q = H.gemm_inputs(0, m, k, n)
    H.poison(eng)
    got = eng.tile_dgemm_acc(a, b, c0.copy(order="F"))
    _same(got, H.expected(0, q, q["c0"]))


@SHAPE
@pytest.mark.parametrize("with_add", [False, True], ids=["plain", "add"])
def test_sgemm_epilogue_after_poison(eng, m, k, n, with_add):
    a, b, _, add, q = H.gemm_inputs(1, m, k, n)
    H.poison(eng, fused=True)
    got = eng.sgemm_transpose_add(a, b, add_c=add if with_add else None)
    _same(got, H.expected_t(q, with_add))


@FP
@pytest.mark.parametrize("entry", ["summa", "kres"])
@pytest.mark.parametrize("m,k,n", H.SUMMA_SHAPES)
def test_summa_host_after_poison(eng, fp32, entry, m, k, n):
    c = S.SummaCase(fp32, 1, 1, m, k, n, 0)
    res = S.run_real_host(eng, c, entry, poison=H.poison)
    assert res["rc"] == 0 and res["ok"], res
    assert not res["sentinel_inside"] and res["launches"] == 1, res


# ---------------------------------------------------------------------------
# the flat entries, bit for bit against numpy on integer-valued data
def _flat(rows, cols, seed):
    return np.asfortranarray(H.flat_ints(rows, cols, seed).astype(np.float64))


@pytest.mark.parametrize("op", ["add", "muls"])
def test_map_after_poison(eng, op):
    a, b = _flat(H.MAP_N, 1, 1), _flat(H.MAP_N, 1, 2)
    H.poison(eng)
    if op == "add":
        _same(eng.map_op("add", a, b), a + b)
    else:
        _same(eng.map_op("muls", a, scalar=3.0), a * 3.0)


def test_sum_after_poison(eng):
    q = H.flat_ints(H.SUM_N, 1, 3)
    H.poison(eng)
    assert eng.sum(q.astype(np.float64)) == float(q.sum())


def test_transpose_after_poison(eng):
    a = _flat(*H.TRANSPOSE_SHAPE, 4)
    H.poison(eng)
    _same(eng.transpose(a), np.asfortranarray(a.T))


def test_dgemv_after_poison(eng):
    m, n = H.GEMV_SHAPE
    qa, qx = H.flat_ints(m, n, 5), H.flat_ints(n, 1, 6)[:, 0]
    H.poison(eng)
    y = eng.dgemv(qa.astype(np.float64), qx.astype(np.float64))
    _same(y, (qa @ qx).astype(np.float64))


# ---------------------------------------------------------------------------
def test_image_size_refusals_then_exact(eng):
    """An image whose byte size leaves int64 is MX_ENOMEM before any copy:
    the host pointers here are one element long."""
    lib, ctx = E.lib(), eng._ctx
    x = np.zeros(1, dtype=np.float64)
    big = 1 << 31
    for fp32 in (0, 1):
        for ta, tb in H.FORMS:
            assert lib.mx_gemm_op(ctx, fp32, ta, tb, big, 16, big, _vp(x),
                                  _vp(x), _vp(x)) == ENOMEM
        assert lib.mx_transpose(ctx, fp32, big, big, _vp(x), _vp(x)) == ENOMEM
    assert lib.mx_transpose(ctx, 0, 1 << 40, 1 << 40, _vp(x), _vp(x)) == ENOMEM
    muls = Engine.OPS["muls"]
    assert lib.mx_map(ctx, muls, 0, 1 << 61, _vp(x), None, 2.0,
                      _vp(x)) == ENOMEM
    assert lib.mx_map(ctx, muls, 1, 1 << 62, _vp(x), None, 2.0,
                      _vp(x)) == ENOMEM
    # the engine is as it was: a ragged multiply right after is exact
    a, b, _, _, q = H.gemm_inputs(0, 129, 17, 127)
    _same(eng.dgemm(a, b), H.expected(0, q))
