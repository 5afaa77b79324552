# Exact-arithmetic GEMM test helper (shared by test_gpu_gemm_exact.py,
# gemm_cfg_worker.py and the CPU-only test_exact_inputs.py).
#
# Idea: feed the MFMA kernels small signed INTEGER data, chosen so that
# every product and every partial sum -- in ANY accumulation order, fused
# or not -- is exactly representable. A correct kernel must then return
# the mathematically exact product bit for bit, so the assertion is
# assert_array_equal instead of a max-norm tolerance, and one dropped
# k-term, swapped lane/chunk/tile or stale LDS buffer is always visible.
#
# Representability bounds (asserted from the generated data in
# test_exact_inputs.py):
#
#   fp32  entries are integers in [-15, 15], K <= 512.
#         |a*b| <= 225 < 2^8; any partial sum of <= 512 products is an
#         integer with |s| <= 225*512 = 115200; with the beta=1 seed
#         |C0| <= 15 the bound is 115215 < 2^17. fp32 represents every
#         integer up to 2^24 exactly, so no operation ever rounds.
#
#   fp64  entries are q * 2^-19 with integer |q| <= 2^19, K <= 4096.
#         A product is (q1*q2) * 2^-38 with |q1*q2| <= 2^38; any partial
#         sum of <= 2^12 products is an integer multiple of 2^-38 with
#         magnitude <= 2^50 units. The beta=1 seed C0 = q * 2^-19
#         = (q * 2^19) * 2^-38 adds <= 2^38 units: total < 2^51 units.
#         fp64 carries 53 significand bits, so every such multiple of
#         2^-38 is exact (38 + 12 + 1 = 51 <= 53 bits).
#
# The reference A.astype(f64) @ B.astype(f64) is exact on these inputs
# for the same reason (BLAS order/FMA do not matter); the CPU test pins
# that once against an int64 matmul.
import functools
from collections import namedtuple

import numpy as np

from oracle import gen_uniform_u64

F32_AMAX = 15            # fp32 entries: integers in [-15, 15]
F32_KMAX = 512
F64_QBITS = 19           # fp64 entries: q * 2^-19, |q| <= 2^19
F64_QMAX = 1 << F64_QBITS
F64_KMAX = 4096
PAD = 16                 # extra pitch elements: 64/128 bytes, keeps 16B align

# Sentinels. beta=0: the whole C buffer is a NaN with a recognisable
# payload; beta=1: the pad rows / trailing column hold a finite value no
# exact result can take (results are < 2^17 resp. < 2^13 in magnitude).
NAN_BITS = {np.float64: np.uint64(0x7FF80000DEADBEEF),
            np.float32: np.uint32(0x7FC0BEEF)}
UINT = {np.float64: np.uint64, np.float32: np.uint32}
FINITE_SENTINEL = -1.5 * 2.0 ** 100

Case = namedtuple("Case", "fp32 beta M N K")


def case_id(c):
    return f"{'f32' if c.fp32 else 'f64'}-b{c.beta}-{c.M}x{c.N}x{c.K}"


def dtype_of(fp32):
    return np.float32 if fp32 else np.float64


@functools.lru_cache(maxsize=None)
def int_matrix(rows, cols, seed, amax):
    """int64 matrix, entries pseudo-random per (r, c, seed) in
    [-amax, amax]: the oracle's splitmix stream (col-major linear index)
    reduced modulo the range and shifted."""
    z = gen_uniform_u64(seed, 0, rows * cols)
    q = (z % np.uint64(2 * amax + 1)).astype(np.int64) - amax
    q = np.asfortranarray(q.reshape((cols, rows)).T)
    q.setflags(write=False)
    return q


def exact_matrix(rows, cols, seed, fp32):
    """(values, q): values in the kernel's dtype, q the int64 numerators
    (values == q for fp32, values == q * 2^-19 for fp64)."""
    if fp32:
        q = int_matrix(rows, cols, seed, F32_AMAX)
        return np.asfortranarray(q.astype(np.float32)), q
    q = int_matrix(rows, cols, seed, F64_QMAX)
    return np.asfortranarray(q.astype(np.float64) * 2.0 ** -F64_QBITS), q


def _seeds(c):
    base = (c.M * 1000003 + c.N * 10007 + c.K * 101 + c.fp32 * 7 + c.beta)
    return base + 0xA000, base + 0xB000, base + 0xC000


@functools.lru_cache(maxsize=None)
def gemm_inputs(c):
    """(A, B, C0, ref) for a case; ref = exact C0*beta + A@B in float64
    (computed once per case and never modified)."""
    assert c.K <= (F32_KMAX if c.fp32 else F64_KMAX)
    sa, sb, sc = _seeds(c)
    a, _ = exact_matrix(c.M, c.K, sa, c.fp32)
    b, _ = exact_matrix(c.K, c.N, sb, c.fp32)
    c0, _ = exact_matrix(c.M, c.N, sc, c.fp32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    if c.beta:
        ref = ref + c0.astype(np.float64)
    for x in (a, b, c0, ref):
        x.setflags(write=False)
    return a, b, c0, ref


# ---------------------------------------------------------------------------
# case tables
GRIDS = [(1, 1), (1, 9), (9, 1), (8, 8), (9, 9), (3, 17), (17, 3)]
BETA1_GRIDS = [(1, 1), (9, 9), (3, 17)]
K_TILES = [16, 32, 48, 80]          # ntiles 1, 2, 3, 5 at BK=16
EPI_GRIDS = [(1, 1), (9, 9), (3, 17), (17, 3)]
EPI_KS = [16, 48]


def default_cases():
    out = []
    for fp32 in (0, 1):
        for nbm, nbn in GRIDS:
            out.append(Case(fp32, 0, 128 * nbm, 128 * nbn, 32))
        for nbm, nbn in BETA1_GRIDS:
            out.append(Case(fp32, 1, 128 * nbm, 128 * nbn, 32))
        for k in K_TILES:
            for beta in (0, 1):
                out.append(Case(fp32, beta, 256, 256, k))
    return out


def config_cases(env):
    """The default table plus the shapes a MARLIN_GEMM_CFG variant needs:
    bk32 -> K=64, 96 (2 and 3 BK=32 tiles; K=48/80 already in the table
    must fall back to BK=16); bm256 -> M=2304 (nbm=9 at BM=256) and
    M=384 (must fall back to BM=128); M=256 is already in the table."""
    out = default_cases()
    cfg = env.get("MARLIN_GEMM_CFG", "")
    extra = []
    if cfg.startswith("bk"):
        extra = [(256, 256, 64), (256, 256, 96)]
    elif cfg.startswith("bm"):
        extra = [(2304, 1152, 32), (384, 256, 32)]
    for (m, n, k) in extra:
        for fp32 in (0, 1):
            for beta in (0, 1):
                out.append(Case(fp32, beta, m, n, k))
    assert len(set(out)) == len(out)
    return out


def expected_config(env, c):
    """Restatement of the launcher's variant selection (mx_gemm_select of
    gemm_launch_policy.h; test_gemm_launch_policy.py compares the two on
    the CPU): what mx_last_gemm_config must report for case c under env."""
    cfg = env.get("MARLIN_GEMM_CFG", "")
    bk32 = cfg.startswith("bk") and c.K % 32 == 0
    bm256 = cfg.startswith("bm") and not c.fp32 and c.M % 256 == 0
    bandw = int(env.get("MARLIN_GEMM_BAND", "8"))
    if bandw < 1:
        bandw = 8
    band = min(c.N // 128, bandw)
    if env.get("MARLIN_GEMM_REMAP", "").startswith("b"):
        band = -band
    return {
        "is_fp32": int(c.fp32), "beta_one": int(c.beta),
        "bk": 32 if (bk32 and not bm256) else 16,
        "bm": 256 if bm256 else 128,
        "waves": 8 if (bk32 or bm256) else 4,
        "band": band,
        "phase_mask": int(env.get("MARLIN_GEMM_PHASE", "0")),
    }


# ---------------------------------------------------------------------------
# device runs
def _bits(x):
    return np.ascontiguousarray(x).view(UINT[x.dtype.type])


def _first_bad(got, ref):
    bad = np.argwhere(got != ref)
    return [int(v) for v in bad[0]] if len(bad) else None


def _check_image(img, rows, cols, ref, sentinel_bits):
    """img: (ld x cols+1) downloaded C image. Returns the result dict:
    interior exact, no sentinel inside, pad rows + trailing column still
    the sentinel bit for bit."""
    inner = img[:rows, :cols]
    ibits = _bits(inner)
    first_bad = _first_bad(inner.astype(np.float64), ref)
    pad_rows = _bits(img[rows:, :])
    pad_col = _bits(img[:, cols:])
    return {
        "ok": first_bad is None,
        "first_bad": first_bad,
        "sentinel_inside": bool((ibits == sentinel_bits).any()),
        "pad_ok": bool((pad_rows == sentinel_bits).all()
                       and (pad_col == sentinel_bits).all()),
    }


def _padded(x, ld, extra_cols, fill):
    """x (r x c) embedded in an (ld x c+extra_cols) col-major image whose
    every other element is `fill` (a dtype scalar, NaN payload kept)."""
    img = np.empty((ld, x.shape[1] + extra_cols), dtype=x.dtype, order="F")
    img.view(UINT[x.dtype.type])[...] = fill.view(UINT[x.dtype.type])
    img[:x.shape[0], :x.shape[1]] = x
    return img


def _nan(dt):
    return NAN_BITS[dt].view(dt)


def _filled(rows, cols, fill):
    """(rows x cols) col-major image with every element `fill`'s bits."""
    img = np.empty((rows, cols), dtype=fill.dtype, order="F")
    img.view(UINT[fill.dtype.type])[...] = fill.view(UINT[fill.dtype.type])
    return img


def _dev(eng, img, bufs):
    d = eng.alloc(img.nbytes)
    bufs.append(d)
    eng.upload(d, img, img.nbytes)
    return d


def run_gemm_case(eng, c):
    """Run one case through mx_gemm_device_ex with pitches larger than
    the dims (lda = M+16, ldb = K+16, ldc = M+16). A/B pad rows hold NaN,
    so a kernel that strays into them poisons the result."""
    from marlin_amd import engine as E
    dt = dtype_of(c.fp32)
    a, b, c0, ref = gemm_inputs(c)
    lda, ldb, ldc = c.M + PAD, c.K + PAD, c.M + PAD
    nan = _nan(dt)
    sentinel = dt(FINITE_SENTINEL) if c.beta else nan
    cimg = (_padded(c0, ldc, 1, sentinel) if c.beta
            else _filled(ldc, c.N + 1, nan))
    bufs = []
    try:
        dA = _dev(eng, _padded(a, lda, 0, nan), bufs)
        dB = _dev(eng, _padded(b, ldb, 0, nan), bufs)
        dC = _dev(eng, cimg, bufs)
        rc = E.lib().mx_gemm_device_ex(eng._ctx, int(c.fp32), int(c.beta),
                                       c.M, c.K, c.N, dA, lda, dB, ldb, dC,
                                       ldc)
        if rc != 0:
            return {"ok": False, "rc": rc, "first_bad": None,
                    "sentinel_inside": False, "pad_ok": False, "cfg": None}
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        res = _check_image(got, c.M, c.N, ref, sentinel.view(UINT[dt]))
        res["rc"] = 0
        res["cfg"] = eng.last_gemm_config()
        return res
    finally:
        for d in bufs:
            eng.free(d)


@functools.lru_cache(maxsize=None)
def epilogue_inputs(M, N, K):
    c = Case(1, 0, M, N, K)
    a, b, _, ref = gemm_inputs(c)
    add, _ = exact_matrix(N, M, _seeds(c)[2] + 0x1000, True)
    add.setflags(write=False)
    return a, b, add, ref


def run_epilogue_case(eng, M, N, K, with_add):
    """C[N x M] = (A*B)^T (+ addC) through mx_sgemm_epilogue_device with
    lda = M+16, ldb = K+16, ldc = N+16; C prefilled with the NaN
    sentinel, addC pad rows NaN."""
    from marlin_amd import engine as E
    dt = np.float32
    a, b, add, ref = epilogue_inputs(M, N, K)
    ref_t = ref.T + add.astype(np.float64) if with_add else ref.T
    lda, ldb, ldc = M + PAD, K + PAD, N + PAD
    nan = _nan(dt)
    cimg = _filled(ldc, M + 1, nan)
    bufs = []
    try:
        dA = _dev(eng, _padded(a, lda, 0, nan), bufs)
        dB = _dev(eng, _padded(b, ldb, 0, nan), bufs)
        dC = _dev(eng, cimg, bufs)
        dAdd = _dev(eng, _padded(add, ldc, 1, nan), bufs) if with_add else None
        rc = E.lib().mx_sgemm_epilogue_device(eng._ctx, M, K, N, dA, lda, dB,
                                              ldb, dC, ldc, dAdd)
        if rc != 0:
            return {"ok": False, "rc": rc, "first_bad": None,
                    "sentinel_inside": False, "pad_ok": False}
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        res = _check_image(got, N, M, ref_t, nan.view(UINT[dt]))
        res["rc"] = 0
        return res
    finally:
        for d in bufs:
            eng.free(d)
