# Case tables of the exact host-entry tests (test_gpu_host_entries_exact.py
# on the GPU, test_host_cases_cpu.py for the claims made here).
#
# The host-buffer entries stage into workspaces that are cached per context
# and shared by all of them, and the kernels read the pad of an image.
# Every case therefore runs right after a POISON call on the same engine,
# which leaves NaN in every byte the case's images will occupy; a pad that
# staging did not zero, or an unpadded image the copy did not define, then
# reaches the product as NaN * 0 = NaN and the exact comparison fails.
#
# Inputs are _exact.exact_matrix data inside the bounds stated in
# _exact.py (fp32: integers in [-15, 15], K <= 512; fp64: q * 2^-19,
# K <= 4096; the beta seed and add_c inside the same bounds), so every
# expected value is computed in int64 and compared with assert_array_equal.
import functools

import numpy as np

import _exact
from _exact import dtype_of

# (m, k, n)
SHAPES = [
    (1, 1, 1),
    (129, 17, 127),
    (257, 15, 1),
    (128, 16, 128),      # nothing padded: no memset, the copy defines all
    (128, 17, 128),      # only k ragged
    (130, 16, 128),      # only m ragged
    (128, 16, 5),        # only n ragged
]
FORMS = [(0, 0), (1, 0), (0, 1), (1, 1)]
# the plain entries by name, one ragged shape each
NAMED = {"mx_dgemm": (0, (129, 17, 127)), "mx_sgemm": (1, (257, 15, 1))}
# one-rank SUMMA host entries: the table above, and two with k raised to 40
# (one panel at the default width: the staging is under test, not the loop)
SUMMA_SHAPES = SHAPES + [(128, 40, 128), (129, 40, 127)]

# The poison multiply: NaN x NaN in fp64 through the same engine. Its A, B
# and C images are unpadded, so the NaN operands fill wsA and wsB and the
# NaN product fills wsC. For the fused-epilogue cases an fp32 NaN
# sgemm_transpose_add of the same padded size fills wsPA[0] with its add_c.
POISON = (384, 32, 384)


def roundup(x, a):
    return (x + a - 1) // a * a


def gemm_image_bytes(m, k, n, elem):
    """Bytes of the A, B, C (and add_c = C) images of an m x k x n host
    multiply in any op form: mp x kp, kp x np, mp x np elements."""
    mp, kp, np_ = roundup(m, 128), roundup(k, 16), roundup(n, 128)
    return mp * kp * elem, kp * np_ * elem, mp * np_ * elem


def poison_bytes():
    """Bytes the poison call leaves NaN at the start of wsA, wsB, wsC (fp64)
    and of wsPA[0] (fp32 add_c)."""
    a, b, c = gemm_image_bytes(*POISON, 8)
    return a, b, c, gemm_image_bytes(*POISON, 4)[2]


@functools.lru_cache(maxsize=None)
def _nan_operands(fp32):
    dt = dtype_of(fp32)
    m, k, n = POISON
    return (np.full((m, k), np.nan, dtype=dt, order="F"),
            np.full((k, n), np.nan, dtype=dt, order="F"),
            np.full((n, m), np.nan, dtype=dt, order="F"))


def poison(eng, fused=False):
    a, b, _ = _nan_operands(0)
    assert np.isnan(eng.dgemm(a, b)).all()
    if fused:
        a, b, add = _nan_operands(1)
        assert np.isnan(eng.sgemm_transpose_add(a, b, add_c=add)).all()


def _seed(fp32, m, k, n):
    return m * 1000003 + k * 10007 + n * 101 + fp32 * 7 + 0x40570000


def from_q(q, fp32, scale_bits):
    """The dtype array whose value is q (fp32) or q * 2^-scale_bits (fp64),
    exactly: |q| stays below 2^24 resp. 2^53 in every use here."""
    if fp32:
        return np.asfortranarray(q.astype(np.float32))
    return np.asfortranarray(q.astype(np.float64) * 2.0 ** -scale_bits)


@functools.lru_cache(maxsize=None)
def gemm_inputs(fp32, m, k, n):
    """(A, B, C0, add, q): exact op(A) m x k, op(B) k x n, the beta seed C0
    m x n, add_c n x m, and q = dict of the int64 numerators (a, b, c0, add,
    prod = a @ b). Arrays are read-only."""
    assert k <= (_exact.F32_KMAX if fp32 else _exact.F64_KMAX)
    s = _seed(fp32, m, k, n)
    a, qa = _exact.exact_matrix(m, k, s + 1, fp32)
    b, qb = _exact.exact_matrix(k, n, s + 2, fp32)
    c0, qc = _exact.exact_matrix(m, n, s + 3, fp32)
    add, qadd = _exact.exact_matrix(n, m, s + 4, fp32)
    for x in (a, b, c0, add):
        x.setflags(write=False)
    return a, b, c0, add, {"a": qa, "b": qb, "c0": qc, "add": qadd,
                           "prod": qa @ qb}


def product_q(fp32, q, seed_q=None):
    """int64 numerator of A @ B (+ seed) in units of 1 (fp32) or 2^-38
    (fp64, where a seed q * 2^-19 is q * 2^19 units)."""
    out = q["prod"]
    if seed_q is not None:
        out = out + (seed_q if fp32 else seed_q * (1 << _exact.F64_QBITS))
    return out


def expected(fp32, q, seed_q=None):
    return from_q(product_q(fp32, q, seed_q), fp32, 2 * _exact.F64_QBITS)


def expected_t(q, with_add):
    """(A @ B)^T (+ add_c) of the fused epilogue (fp32 only)."""
    return from_q(q["prod"].T + (q["add"] if with_add else 0), 1, 0)


def stored(x, trans):
    """The operand as the entry takes it: op(X) = X^T where trans."""
    return np.asfortranarray(x.T) if trans else x


# flat entries: element counts below the poison's 12288 doubles, so the
# previous call's image was larger; odd, and no multiple of a block
MAP_N = 4999
SUM_N = 4999
TRANSPOSE_SHAPE = (37, 129)
GEMV_SHAPE = (129, 65)
FLAT_AMAX = 1000          # |entries|: sums stay far below 2^53 (and 2^24)


@functools.lru_cache(maxsize=None)
def flat_ints(rows, cols, seed):
    return _exact.int_matrix(rows, cols, 0x0F1A7000 + seed, FLAT_AMAX)
