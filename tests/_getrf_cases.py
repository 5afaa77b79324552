# Shapes, inputs and device runs of the LU factorisation tests
# (test_gpu_getrf.py, test_gpu_getrf_consumers.py), the numpy restatement of
# the block-pivoted elimination they compare with, and the Python
# restatement of the entry's argument check that test_getrf_plan.py compares
# with the C++ (marlin_amd/csrc/getrf_plan.h). No GPU is needed to import
# this; test_getrf_cases.py proves the inputs on the CPU.
#
# Exact data: A = P^T (L U). L is unit-lower with entries in {0, +-1/4,
# +-1/2}, U upper with integer entries in [-4, 4] and a diagonal in
# +-{1, 2, 4}, P a permutation that maps each 128-block to itself. Every
# partial sum of an entry of L U is a multiple of 1/4 below 2 n 4 = 2400 at
# n = 300, exact in fp32 and fp64, so A is exact, and so is every
# intermediate of the elimination, of the two substitutions and of the
# k = 128 GEMM, in any order (each is a partial sum of the same products).
# Every multiplier is a (multiple of 1/4) * u_jj / u_jj with u_jj a power of
# two. At step j the candidates of column j are u_jj (the intended row) and
# l_ij u_jj with |l_ij| <= 1/2: the intended pivot is the unique maximum. A
# correct factorisation returns packed L\U and P's array bit for bit, but
# for the sign of an exact zero (zero_sign_dropped below).
import functools

import numpy as np

from _exact import PAD, UINT, _dev, _filled, _nan, dtype_of

EINVAL = -4
W = 128
ORDERS = [1, 127, 128, 129, 300]
LVALS = np.array([0, 0.25, -0.25, 0.5, -0.5])
DVALS = np.array([1.0, -1, 2, -2, 4, -4])


def r128(x):
    return (x + W - 1) // W * W


# ---------------------------------------------------------------------------
# the argument check, restated (aliasing aside: it needs device pointers)
def check(w, fp32, n, bytes_a, lda, bytes_p, info_null=False):
    """(rc, empty) of mx_getrf_check for two distinct, disjoint buffers of
    the given sizes. Python integers: nothing can overflow."""
    if fp32 not in (0, 1) or n < 0 or info_null:
        return EINVAL, False
    if n == 0:
        return 0, True
    np_ = (n + w - 1) // w * w
    if np_ > 2 ** 31 - 1:
        return EINVAL, False
    elem = 4 if fp32 else 8
    if lda < np_ or lda % (16 // elem) or bytes_a < 0 or bytes_p < 0:
        return EINVAL, False
    if (np_ - 1) * lda + np_ > bytes_a // elem or np_ * 4 > bytes_p:
        return EINVAL, False
    return 0, False


# ---------------------------------------------------------------------------
# the elimination, restated: unblocked over the whole matrix, the pivot of
# column j searched among the rows of j's block only
def block_lu(a, w=W, tie_cols=None):
    """(packed L\\U, piv, info) in a's element type: right-looking
    elimination column by column with WHOLE rows swapped; the pivot is the
    first row of largest |a| (a NaN counts as -1) among rows [j, end of j's
    w-block); a zero pivot leaves its column unscaled and sets info to its
    1-based column if it is the first. a[piv] == L @ U. tie_cols, a list,
    receives every column whose largest magnitude occurred more than once."""
    a = np.array(a, order="F", copy=True)
    n = a.shape[0]
    piv = np.arange(n)
    info = 0
    with np.errstate(all="ignore"):
        for j in range(n):
            end = min((j // w + 1) * w, n)
            col = a[j:end, j]
            key = np.where(np.isnan(col), -1, np.abs(col))
            p = j + int(np.argmax(key))          # the first of the maxima
            if tie_cols is not None and np.sum(key == key.max()) > 1:
                tie_cols.append(j)
            if p != j:
                a[[j, p], :] = a[[p, j], :]
                piv[[j, p]] = piv[[p, j]]
            d = a[j, j]
            if d == 0:
                info = info or j + 1
            else:
                a[j + 1:, j] = a[j + 1:, j] / d
            a[j + 1:, j + 1:] -= np.outer(a[j + 1:, j], a[j, j + 1:])
    return a, piv, info


# ---------------------------------------------------------------------------
# the diagonal kernel's arithmetic, restated (test_gpu_diag_bits.py compares
# the device with it bit for bit on rounding data; test_diag_bits_cpu.py
# proves it against mx_getrf_eliminate of marlin_amd/csrc/getrf_plan.h)
MODELS = ("fused", "unfused", "reciprocal")


def eliminate_restated(block, nv, model="fused"):
    """(block after, perm, first_zero) of mx_getrf_eliminate on the leading
    nv x nv part of a square block, in its element type: column by column,
    the pivot by block_lu's key rule (largest |a|, a NaN counts as -1, the
    first of equal keys), the multiplier l = a / pivot (one division), the
    update fma(-l, u, a) (one rounding) over the whole trailing block at
    once. perm[g] is the source row of output row g, first_zero the 1-based
    column of the first exactly-zero pivot or 0. `model` degrades it on
    purpose: "unfused" rounds the product before the subtraction,
    "reciprocal" multiplies by 1 / pivot."""
    import _fma
    assert model in MODELS
    a = np.array(block, order="F", copy=True)
    dt = a.dtype.type
    perm = np.arange(a.shape[0])
    first_zero = 0
    with np.errstate(all="ignore"):
        for j in range(nv):
            col = a[j:nv, j]
            key = np.where(np.isnan(col), -1, np.abs(col))
            p = j + int(np.argmax(key))          # the first of the maxima
            if p != j:
                a[[j, p], :nv] = a[[p, j], :nv]
                perm[[j, p]] = perm[[p, j]]
            d = a[j, j]
            if d == 0:
                first_zero = first_zero or j + 1
            elif model == "reciprocal":
                a[j + 1:nv, j] = a[j + 1:nv, j] * (dt(1) / d)
            else:
                a[j + 1:nv, j] = a[j + 1:nv, j] / d
            l, u = a[j + 1:nv, j][:, None], a[j, j + 1:nv][None, :]
            if dt is np.float64:
                assert _fma.in_range64(l[np.isfinite(l)], u[np.isfinite(u)]), \
                    "outside the range fma64 is valid in"
            if model == "unfused":
                a[j + 1:nv, j + 1:nv] = a[j + 1:nv, j + 1:nv] - l * u
            else:
                a[j + 1:nv, j + 1:nv] = _fma.fma(-l, u, a[j + 1:nv, j + 1:nv])
    return a, perm, first_zero


def same_bits(got, want):
    """Bit for bit after -0 -> +0, a NaN matching any NaN: the comparison
    of the rounding-data tests. Returns the (row, col) of the mismatches."""
    U = UINT[got.dtype.type]
    g, w = zero_sign_dropped(got), zero_sign_dropped(want)
    gn, wn = np.isnan(g), np.isnan(w)
    return np.argwhere((gn != wn) | (~gn & (g.view(U) != w.view(U))))


@functools.lru_cache(maxsize=None)
def normal_problem(fp32, n, scale_exp=0):
    """A n x n in the element type: standard normal, nothing dominant, times
    2^scale_exp (exact but where it leaves the normal range, which is the
    point of scale_exp = -130 in fp32: entries, updates and results are
    subnormal there, the multipliers stay O(1))."""
    dt = dtype_of(fp32)
    rng = np.random.RandomState(_seed(5, fp32, n))
    a = rng.standard_normal((n, n)).astype(dt)
    a = np.ldexp(a, scale_exp).astype(dt)
    return _frozen(np.asfortranarray(a))[0]


NAN_N = 128


@functools.lru_cache(maxsize=None)
def nan_problem(fp32):
    """(A, r): normal_problem at n = 128 with one NaN in column 0 at a row r
    that is not column 0's pivot row. The NaN is never chosen while another
    entry remains: row r turns NaN whole at step 0 (its multiplier is NaN),
    is passed over at every later column and ends at the bottom, and no
    other row ever meets it."""
    a = np.array(normal_problem(fp32, NAN_N))
    r = 5 if int(np.argmax(np.abs(a[:, 0]))) != 5 else 6
    a[r, 0] = np.nan
    return _frozen(a)[0], r


@functools.lru_cache(maxsize=None)
def inf_problem(fp32):
    """(A, r1, r2): normal_problem at n = 128 with +inf at (r1, 0) and -inf
    at (r2, 0), r1 < r2: two candidates of equal key, the lowest row wins.
    Row r2's multiplier is -inf / inf = NaN, so it goes the way of
    nan_problem's row; every other multiplier of column 0 is a zero."""
    a = np.array(normal_problem(fp32, NAN_N))
    r1, r2 = 40, 90
    a[r1, 0], a[r2, 0] = np.inf, -np.inf
    return _frozen(a)[0], r1, r2


def block_lu_solve(a, b, w=W):
    """x with a x = b through block_lu and two substitutions, everything in
    a's element type: the host solve the device one is compared with."""
    import scipy.linalg
    lu, piv, info = block_lu(a, w)
    assert info == 0
    y = scipy.linalg.solve_triangular(lu, b[piv], lower=True,
                                      unit_diagonal=True)
    return scipy.linalg.solve_triangular(lu, y, lower=False).astype(a.dtype)


# ---------------------------------------------------------------------------
# inputs
def _seed(*key):
    s = 0x6E7F
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return s


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


def block_perm(n, rng, w=W):
    """P's array: piv[g] is the row of A that holds row g of L U; each
    w-block maps to itself."""
    p = np.arange(n)
    for o in range(0, n, w):
        ln = min(w, n - o)
        p[o:o + ln] = o + rng.permutation(ln)
    return p


def _factors(n, rng):
    L = np.tril(LVALS[rng.randint(0, 5, size=(n, n))], -1) + np.eye(n)
    U = np.triu(rng.randint(-4, 5, size=(n, n)).astype(np.float64), 1)
    U[np.arange(n), np.arange(n)] = DVALS[rng.randint(0, 6, size=n)]
    return L, U


def _assemble(L, U, p):
    """(A, packed L\\U, p) in float64 with A[p] == L @ U."""
    n = L.shape[0]
    a = np.empty((n, n), order="F")
    a[p, :] = L @ U
    packed = np.asfortranarray(np.tril(L, -1) + U)
    return _frozen(a, packed, p)


@functools.lru_cache(maxsize=None)
def exact_problem(n):
    rng = np.random.RandomState(_seed(1, n))
    L, U = _factors(n, rng)
    return _assemble(L, U, block_perm(n, rng))


def positions_at(p, c):
    """pos[r] = the row of L U that sits at row r of the working matrix
    when column c's pivot is chosen, given that every earlier step brought
    the intended row up (which the exact data guarantees)."""
    pos = np.empty(len(p), dtype=np.int64)
    pos[p] = np.arange(len(p))           # row p[g] of A holds row g
    for j in range(c):
        q = int(np.nonzero(pos == j)[0][0])
        pos[[j, q]] = pos[[q, j]]
    return pos


TIE_N, TIE_COL = 129, 40


@functools.lru_cache(maxsize=None)
def tie_problem():
    """n = 129. Column TIE_COL of L holds +-1 in three rows that, when that
    column's pivot is chosen, sit BELOW the intended row: the candidates
    then tie in magnitude and the lowest row index must win, which is the
    intended one, so the data stay exact and the expected result (taken
    from block_lu) is again packed L\\U and P's array."""
    n, c = TIE_N, TIE_COL
    rng = np.random.RandomState(_seed(2, n))
    L, U = _factors(n, rng)
    p = block_perm(n, rng)
    pos = positions_at(p, c)
    at = int(np.nonzero(pos == c)[0][0])
    below = [int(g) for g in pos[at + 1:W] if g > c]
    assert at < W - 8 and len(below) >= 3, "pick another seed: no room below"
    for g, s in zip(below[:3], (1.0, -1.0, 1.0)):
        L[g, c] = s
    return _assemble(L, U, p)


ZERO_N, ZERO_COL = 129, 70              # the 1-based global column


@functools.lru_cache(maxsize=None)
def zero_pivot_problem():
    """n = 129. u_jj = 0 at the 0-based column j = ZERO_COL - 1, and column
    j of L is zero below its diagonal: after the elimination of the columns
    before it, column j is zero on and below the diagonal inside its block,
    the pivot is exactly zero, and skipping its (zero) multipliers changes
    nothing, so block 0 goes on exactly as intended. The rows below block 0
    are divided by that zero when L21 is formed, so only the columns before
    it are comparable. With every candidate zero the row already AT the
    diagonal stays (the lowest index), so P is arranged to have the
    intended row there when that column's turn comes."""
    n, j = ZERO_N, ZERO_COL - 1
    rng = np.random.RandomState(_seed(3, n))
    L, U = _factors(n, rng)
    U[j, j] = 0.0
    L[j + 1:, j] = 0.0
    p = block_perm(n, rng)
    g = int(positions_at(p, j)[j])       # the row that would sit there
    p[[j, g]] = p[[g, j]]                # neither is sought before step j
    assert positions_at(p, j)[j] == j
    return _assemble(L, U, p)


@functools.lru_cache(maxsize=None)
def rounding_problem(fp32, n, shuffled):
    """(A, src) in the element type: normal data plus n on the diagonal;
    shuffled moves the rows inside each 128-block (row g of A is row src[g]
    of the dominant matrix)."""
    dt = dtype_of(fp32)
    rng = np.random.RandomState(_seed(4, fp32, n))
    d = rng.standard_normal((n, n)) + n * np.eye(n)
    src = block_perm(n, rng) if shuffled else np.arange(n)
    return _frozen(np.asfortranarray(d[src, :].astype(dt)), src)


# ---------------------------------------------------------------------------
# device runs
def a_image(a, lda, dt, poison=True):
    """The device image of A: np x np at pitch lda with zero pads and
    (poison) NaN in the pitch pad, which nothing may read or write."""
    n = a.shape[0]
    np_ = r128(n)
    img = _filled(lda, np_, _nan(dt)) if poison else np.zeros(
        (lda, np_), dtype=dt, order="F")
    img[:np_, :] = 0
    img[:n, :n] = a
    return img


def zero_sign_dropped(x):
    """x with every -0 replaced by +0 and no other bit changed. An exact
    zero multiplier or remainder takes the sign its operands give it (0 / -2
    is -0), which the known factors do not record; nothing else differs
    from a comparison of bits."""
    out = np.array(x, copy=True, order="F")
    out[out == 0] = 0
    return out


def fetch(eng, d, like):
    got = np.empty_like(like)
    eng.download(got, d, got.nbytes)
    return got


def factor_image(eng, fp32, n, img, repeat=1):
    """Upload the image, run mx_getrf_device `repeat` times, each on a
    fresh upload. Returns (rc, info, [(image, piv) after each run], stats);
    piv has a guard entry behind its np, pre-set to -7."""
    np_ = r128(n)
    bufs, outs = [], []
    piv0 = np.full(np_ + 1, -7, dtype=np.int32)
    try:
        dA = _dev(eng, img, bufs)
        dP = _dev(eng, piv0, bufs)
        rc, info, st = 0, None, None
        for it in range(repeat):
            if it:
                eng.upload(dA, img, img.nbytes)
                eng.upload(dP, piv0, piv0.nbytes)
            rc, info = eng.getrf_raw(n, dA, img.shape[0], dP, bool(fp32),
                                     check=False)
            if rc:
                break
            st = eng.stats()
            outs.append((fetch(eng, dA, img), fetch(eng, dP, piv0)))
        return rc, info, outs, st
    finally:
        for d in bufs:
            eng.free(d)


def residual_ratio(fp32, a, lu, piv):
    """max over the components of |A[piv] - L U| / (gamma_n |L| |U|),
    gamma_n = n u / (1 - n u), formed in np.longdouble: <= 1 is the
    componentwise backward-error bound of Gaussian elimination in any
    order of the sums (Higham, Accuracy and Stability, Thm 9.3), which
    blocking and fused multiply-adds only tighten. The longdouble
    evaluation of the residual adds at most n 2^-64 |L| |U|, far below."""
    ld = np.longdouble
    n = a.shape[0]
    u = ld(2.0) ** (-24 if fp32 else -53)
    L = (np.tril(lu, -1) + np.eye(n, dtype=lu.dtype)).astype(ld)
    U = np.triu(lu).astype(ld)
    res = np.abs(a.astype(ld)[piv, :] - L @ U)
    bound = (n * u / (1 - n * u)) * (np.abs(L) @ np.abs(U))
    return float(np.max(res / bound))
