# Shape tables, input builders and the argument-contract restatement for
# the exact tests of the auxiliary kernels and entries (fill_random,
# zero_pad, map, sum, transpose, gemv): shared by test_gpu_aux_exact.py
# (GPU), test_aux_cases.py and test_aux_guards.py (CPU).
#
# Everything the GPU module asserts is a bit comparison. What makes that
# sound, per kernel:
#   gemv       A and x are q * 2^-19 with |q| <= 2^19 (_exact.exact_matrix):
#              any order of <= 4096 products, fused or not, is exact, so
#              A @ x in float64 is the expected value.
#   sum        fp64 q * 2^-19: a sum of <= 2^20 of them is an integer of at
#              most 40 bits in units of 2^-19, exact in any order. fp32
#              integers in [-15, 15], widened exactly by the kernel.
#   transpose, zero_pad  move or clear bits.
#   fill       the oracle states the stream bit for bit.
#   map        IEEE arithmetic in the element type, which numpy states.
# test_aux_cases.py asserts the first two from the generated data.
import functools

import numpy as np

import _exact
from _exact import NAN_BITS, UINT, dtype_of
from oracle import gen_matrix

DTYPES = (np.float64, np.float32)
TAIL = 64                # sentinel elements behind an output region


def elem_of(fp32):
    return 4 if fp32 else 8


# ---------------------------------------------------------------------------
# The argument contract of the auxiliary entries, restated on Python ints
# (marlin_amd/csrc/aux_guards.h is the code; test_aux_guards.py compares
# the two). True = accepted.
def fits(nbytes, elem, off_bytes, ld, rows, cols):
    if off_bytes < 0 or off_bytes > nbytes:
        return False
    if rows == 0 or cols == 0:
        return True
    return (cols - 1) * ld + rows <= (nbytes - off_bytes) // elem


def fill_ok(nbytes, fp32, n):
    return n >= 0 and n * elem_of(fp32) <= nbytes


def zero_pad_ok(nbytes, fp32, rows_total, cols_total, ld, m, n):
    return (0 <= m <= rows_total <= ld and 0 <= n <= cols_total
            and fits(nbytes, elem_of(fp32), 0, ld, rows_total, cols_total))


def transpose_ok(fp32, m, n, bytes_in, bytes_out, same=False):
    return (m >= 0 and n >= 0 and not same
            and m * n * elem_of(fp32) <= min(bytes_in, bytes_out))


def gemv_ok(nbytes, m, n, lda):
    return m >= 1 and n >= 1 and lda >= m and fits(nbytes, 8, 0, lda, m, n)


def copy2d_ok(nbytes, elem, off_bytes, pitch, m, n):
    return (elem in (4, 8) and m >= 1 and n >= 1 and pitch >= m
            and fits(nbytes, elem, off_bytes, pitch, m, n))


def bytes_ok(nbytes, ask):
    return 0 <= ask <= nbytes


def map_op_ok(op):
    return 0 <= op <= 8


# ---------------------------------------------------------------------------
# images with sentinels
def nan_of(dt):
    return NAN_BITS[dt].view(dt)


def bits(x):
    return np.ascontiguousarray(x).view(UINT[x.dtype.type])


def sentinel_vector(n, dt):
    """n elements, every one the NaN sentinel of _exact.NAN_BITS."""
    v = np.empty(n, dtype=dt)
    v.view(UINT[dt])[...] = NAN_BITS[dt]
    return v


def with_tail(x, extra=TAIL):
    """The flat col-major image of x followed by `extra` sentinels."""
    dt = x.dtype.type
    v = sentinel_vector(x.size + extra, dt)
    v[:x.size] = np.asarray(x).reshape(-1, order="F")
    return v


# ---------------------------------------------------------------------------
# gemv: (m, n, lda). 32 column chunks of ceil(n / 32), 256-row blocks.
GEMV_SHAPES = [
    (1, 1, 1),            # smallest case
    (5, 31, 16),          # chunk length 1, n < 32
    (257, 33, 272),       # one live lane in block 2; chunks 17..31 past n
    (256, 128, 256),      # chunk length 4, no tail
    (300, 200, 384),      # chunk length 7, 3-column tail
    (513, 161, 528),      # last chunk length 5, 1-column tail
    (64, 4096, 64),       # long chunks
]


@functools.lru_cache(maxsize=None)
def gemv_inputs(m, n):
    """(A, x, qa, qx, ref): ref = A @ x in float64, exact on these inputs."""
    a, qa = _exact.exact_matrix(m, n, 0x6E3 + 131 * m + n, False)
    xm, qx = _exact.exact_matrix(n, 1, 0x7E4 + 131 * m + n, False)
    x = np.ascontiguousarray(xm[:, 0])
    ref = a @ x
    for v in (x, ref):
        v.setflags(write=False)
    return a, x, qa, qx[:, 0], ref


def gemv_device_image(m, n, lda):
    """A in an lda x (n + 1) image: pad rows [m, lda) and the trailing
    column are NaN, so any read outside m x n poisons y."""
    a = gemv_inputs(m, n)[0]
    return _exact._padded(a, lda, 1, nan_of(np.float64))


# ---------------------------------------------------------------------------
# sum: the 256-thread block and the 1024 x 256 = 262144-thread grid
SUM_NS = [1, 255, 256, 257, 262143, 262144, 262145, 700000]


@functools.lru_cache(maxsize=None)
def sum_inputs(n, fp32):
    """(values, q, expected): expected is the Python-int sum of the
    numerators q, scaled: exact, and what any summation order gives."""
    vals, q = _exact.exact_matrix(n, 1, 0x50B + n + (7 if fp32 else 0), fp32)
    total = sum(q[:, 0].tolist())                 # Python ints: no rounding
    expected = float(total) if fp32 else float(total) * 2.0 ** -_exact.F64_QBITS
    v = np.ascontiguousarray(vals[:, 0])
    v.setflags(write=False)
    return v, q[:, 0], expected


# ---------------------------------------------------------------------------
# transpose: 32 x 32 tiles
TRANSPOSE_SHAPES = [(1, 1), (1, 40), (40, 1), (32, 32), (31, 33), (33, 31),
                    (64, 96)]
PAYLOAD_BITS = {np.float64: np.uint64(0x7FF8000001234567),
                np.float32: np.uint32(0x7FC12345)}
SUBNORMAL_BITS = {np.float64: np.uint64(0x0000000000ABCDEF),
                  np.float32: np.uint32(0x00012345)}
NEG_ZERO_BITS = {np.float64: np.uint64(1 << 63), np.float32: np.uint32(1 << 31)}


@functools.lru_cache(maxsize=None)
def transpose_input(m, n, fp32):
    """gen_matrix data with a NaN payload, -0.0 and a subnormal planted
    (all three where the matrix has room, the payload always)."""
    dt = dtype_of(fp32)
    a = gen_matrix(m, n, seed=0x7A5 + 101 * m + n, dtype=dt)
    flat = a.reshape(-1, order="F").view(UINT[dt]).copy()
    if flat.size >= 3:
        flat[flat.size // 2] = NEG_ZERO_BITS[dt]
        flat[flat.size - 1] = SUBNORMAL_BITS[dt]
    flat[0] = PAYLOAD_BITS[dt]
    a = np.asfortranarray(flat.view(dt).reshape((n, m)).T)
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------------------
# fill_random: the 2048 x 256 = 524288-thread grid
FILL_NS = [1, 1000, 524288, 524289, 1200000]
FILL_SEEDS = [0, 0xA11CE, 2 ** 64 - 1]


@functools.lru_cache(maxsize=None)
def fill_expected(n, seed, fp32):
    v = np.ascontiguousarray(gen_matrix(n, 1, seed, dtype_of(fp32))[:, 0])
    v.setflags(write=False)
    return v


# ---------------------------------------------------------------------------
# zero_pad: (rows_total, cols_total, ld, m, n)
ZERO_PAD_CASES = [
    (256, 256, 256, 200, 150),
    (200, 150, 256, 130, 70),
    (200, 150, 256, 0, 70),
    (200, 150, 256, 130, 0),
    (200, 150, 256, 200, 150),
    (1024, 600, 1040, 1000, 513),     # 614400 elements: more than one grid
]


@functools.lru_cache(maxsize=None)
def zero_pad_images(case, fp32):
    """(image, expected): a random image of ld x (cols_total + 1) with no
    zero in it, and that image with the pads of the rows_total x cols_total
    region set to +0. Rows [rows_total, ld) and the extra column stay."""
    rows_total, cols_total, ld, m, n = case
    dt = dtype_of(fp32)
    img = np.asfortranarray(
        gen_matrix(ld, cols_total + 1, seed=0x2E80 + ld + m, dtype=dt)
        + dt(0.5))
    exp = img.copy(order="F")
    exp[m:rows_total, :cols_total] = 0
    exp[:rows_total, n:cols_total] = 0
    for v in (img, exp):
        v.setflags(write=False)
    return img, exp


# ---------------------------------------------------------------------------
# map: every pair of eight special values, 64 lanes
MAP_OPS = ["add", "sub", "emul", "adds", "subs", "rsubs", "muls", "divs",
           "rdivs"]
MAP_SCALARS = ["one_and_half", "neg_zero", "neg_inf", "min_normal"]


def map_specials(fp32):
    dt = dtype_of(fp32)
    fi = np.finfo(dt)
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, fi.max, fi.tiny,
                     SUBNORMAL_BITS[dt].view(dt)], dtype=dt)


def map_inputs(fp32):
    """(a, b): lane i holds the pair (S[i // 8], S[i % 8])."""
    s = map_specials(fp32)
    return np.repeat(s, 8), np.tile(s, 8)


def map_scalar(name, fp32):
    dt = dtype_of(fp32)
    return {"one_and_half": dt(1.5), "neg_zero": dt(-0.0),
            "neg_inf": dt(-np.inf), "min_normal": np.finfo(dt).tiny}[name]


def map_expected(op, a, b, s):
    """numpy in the element type; s is a scalar of that type."""
    with np.errstate(all="ignore"):
        return {"add": lambda: a + b, "sub": lambda: a - b,
                "emul": lambda: a * b, "adds": lambda: a + s,
                "subs": lambda: a - s, "rsubs": lambda: s - a,
                "muls": lambda: a * s, "divs": lambda: a / s,
                "rdivs": lambda: s / a}[op]()


def is_subnormal(x):
    x = np.asarray(x)
    return (x != 0) & np.isfinite(x) & (np.abs(x) < np.finfo(x.dtype).tiny)
