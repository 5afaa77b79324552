# CPU-only checks around the transposed-operand multiply: the pure shape
# function of Engine.gemm_dd / dgemm / sgemm, the ctypes signatures of the
# three new ABI entries, and that the exact-integer inputs stay exact when
# stored transposed (tests/_exact_op.py).
import ctypes

import numpy as np
import pytest

import _exact
import _exact_op as XO
from marlin_amd import engine as E


@pytest.mark.parametrize("ta,tb,sa,sb,want", [
    (False, False, (130, 45), (45, 200), (130, 45, 200)),
    (True, False, (45, 130), (45, 200), (130, 45, 200)),
    (False, True, (130, 45), (200, 45), (130, 45, 200)),
    (True, True, (45, 130), (200, 45), (130, 45, 200)),
    (True, False, (300, 70), (300, 70), (70, 300, 70)),       # A^T·A
    (False, True, (1, 7), (3, 7), (1, 7, 3)),
])
def test_gemm_op_shape(ta, tb, sa, sb, want):
    assert E.gemm_op_shape(sa, sb, ta, tb) == want


@pytest.mark.parametrize("ta,tb,sa,sb,inner", [
    (False, False, (130, 45), (46, 200), (45, 46)),
    (True, False, (45, 130), (46, 200), (45, 46)),
    (False, True, (130, 45), (200, 46), (45, 46)),
    (True, True, (45, 130), (200, 46), (45, 46)),
    # shapes that multiply untransposed must not pass transposed
    (True, False, (130, 45), (45, 200), (130, 45)),
    (False, True, (130, 45), (45, 200), (45, 200)),
])
def test_gemm_op_shape_mismatch(ta, tb, sa, sb, inner):
    with pytest.raises(ValueError) as ei:
        E.gemm_op_shape(sa, sb, ta, tb)
    msg = str(ei.value)
    assert msg.startswith("Dimension mismatch during matrix-matrix "
                          "multiplication")
    assert msg.endswith(f"{inner[0]} vs {inner[1]}")


def test_ctypes_signatures_of_the_op_entries():
    lib = E.lib()
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert lib.mx_gemm_device_op.restype is i
    assert lib.mx_gemm_device_op.argtypes == [
        vp, i, i, i, i, i64, i64, i64, vp, i64, vp, i64, vp, i64]
    assert lib.mx_gemm_op.restype is i
    assert lib.mx_gemm_op.argtypes == [vp, i, i, i, i64, i64, i64, vp, vp, vp]
    assert lib.mx_last_gemm_op.restype is i
    assert lib.mx_last_gemm_op.argtypes == [
        vp, ctypes.POINTER(i), ctypes.POINTER(i)]
    assert callable(E.Engine.last_gemm_op)


def test_op_table_shape():
    cases = XO.cases()
    # per type: 6 grids + 3 beta-1 grids + 4 K x 2 betas
    assert len(cases) == 2 * (6 + 3 + 8)
    assert len(XO.table()) == 3 * len(cases)
    assert {c.K for c in cases} == {16, 32, 48, 80}
    grids = {(c.M // 128, c.N // 128) for c in cases if c.K == 32}
    assert {(1, 9), (9, 1), (3, 17), (17, 3)} <= grids
    # the largest operand the GPU tests upload
    assert max(max(c.M, c.N) for c in cases) == 2176


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_exact_inputs_stay_exact_when_stored_transposed(fp32):
    """int64 matmul of the numerators recovered from the TRANSPOSED
    stores equals ref: storing an operand transposed changes no value,
    and the stored image is a col-major array of the swapped shape."""
    scale = 1 if fp32 else 2 ** _exact.F64_QBITS
    for c in (_exact.Case(fp32, 0, 384, 2176, 32),
              _exact.Case(fp32, 1, 256, 256, 80)):
        a, b, c0, ref = _exact.gemm_inputs(c)
        sa, sb = XO.stored(a, 1), XO.stored(b, 1)
        assert sa.shape == (c.K, c.M) and sb.shape == (c.N, c.K)
        assert sa.flags.f_contiguous and sb.flags.f_contiguous
        assert sa.dtype == a.dtype and sb.dtype == b.dtype
        qa = np.rint(sa.astype(np.float64) * scale).astype(np.int64)
        qb = np.rint(sb.astype(np.float64) * scale).astype(np.int64)
        assert np.array_equal(qa / scale, sa) and np.array_equal(qb / scale, sb)
        prod = qa.T @ qb.T                       # exact in int64
        if c.beta:
            prod = prod + np.rint(c0.astype(np.float64) * scale).astype(
                np.int64) * scale
        assert np.array_equal(prod.astype(np.float64) / scale ** 2, ref)
        # the untransposed store is the very array
        assert XO.stored(a, 0) is a


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_alias_case_reference(fp32):
    s, ref = XO.alias_inputs(fp32)
    m, k = XO.ALIAS_SHAPE
    assert s.shape == (k, m) and ref.shape == (m, m)
    scale = 1 if fp32 else 2 ** _exact.F64_QBITS
    q = np.rint(s.astype(np.float64) * scale).astype(np.int64)
    assert np.array_equal((q.T @ q).astype(np.float64) / scale ** 2, ref)
    assert np.array_equal(ref, ref.T)


def test_expected_config_of_transposed_forms():
    c = _exact.Case(0, 0, 256, 256, 32)
    plain = XO.expected_config({"MARLIN_GEMM_CFG": "bk32"}, c, 0, 0)
    assert (plain["bk"], plain["waves"]) == (32, 8)
    for ta, tb in XO.FORMS.values():
        for cfg in ("bk32", "bm256"):
            got = XO.expected_config({"MARLIN_GEMM_CFG": cfg}, c, ta, tb)
            assert (got["bk"], got["bm"], got["waves"]) == (16, 128, 4)
        got = XO.expected_config({"MARLIN_GEMM_REMAP": "bands",
                                  "MARLIN_GEMM_PHASE": "1"}, c, ta, tb)
        assert got["band"] == -2 and got["phase_mask"] == 1
