# Exact-integer cases of the transposed-operand GEMM forms (shared by
# test_gpu_gemm_op.py, its child gemm_op_worker.py and the CPU-only
# test_gemm_op_cpu.py). The method, the inputs and the image check are
# tests/_exact.py's: the same A (M x K) and B (K x N) are handed to the
# engine STORED TRANSPOSED where the form says so (A as K x M, B as N x K),
# so the exact product -- and the bit-for-bit assertion -- is unchanged.
import numpy as np

import _exact
from _exact import Case

FORMS = {"tn": (1, 0), "nt": (0, 1), "tt": (1, 1)}

# The non-square grids are the point: a swapped row0/col0, a swapped
# lda/ldb or a wrong pitch in the running pointers cannot survive them.
GRIDS = [(1, 1), (1, 9), (9, 1), (9, 9), (3, 17), (17, 3)]
BETA1_GRIDS = [(1, 1), (9, 9), (3, 17)]
K_TILES = [16, 32, 48, 80]          # 1, 2, 3, 5 tiles: the peeled steps

ALIAS_SHAPE = (384, 48)             # (M = N, K) of the dA == dB case


def cases():
    out = []
    for fp32 in (0, 1):
        for nbm, nbn in GRIDS:
            out.append(Case(fp32, 0, 128 * nbm, 128 * nbn, 32))
        for nbm, nbn in BETA1_GRIDS:
            out.append(Case(fp32, 1, 128 * nbm, 128 * nbn, 32))
        for k in K_TILES:
            for beta in (0, 1):
                out.append(Case(fp32, beta, 256, 256, k))
    assert len(set(out)) == len(out)
    return out


def op_id(form, c):
    return f"{form}-{_exact.case_id(c)}"


def table():
    """[(form, case)] of the whole exact table."""
    return [(f, c) for f in FORMS for c in cases()]


def stored(x, trans):
    """The col-major image the engine is handed for operand x under
    trans: x itself, or a col-major copy of x^T."""
    return np.asfortranarray(x.T) if trans else x


def expected_config(env, c, ta, tb):
    """mx_last_gemm_config of case c run as form (ta, tb) under env: the
    transposed forms exist in the default geometry only."""
    cfg = _exact.expected_config(env, c)
    if ta or tb:
        cfg.update(bk=16, bm=128, waves=4)
    return cfg


def _run(eng, fp32, beta, ta, tb, M, K, N, a_img, lda, b_img, ldb, cimg,
         ref, sentinel, alias):
    """Upload, call mx_gemm_device_op, download and check the C image."""
    from marlin_amd import engine as E
    dt = _exact.dtype_of(fp32)
    bufs = []
    try:
        dA = _exact._dev(eng, a_img, bufs)
        dB = dA if alias else _exact._dev(eng, b_img, bufs)
        dC = _exact._dev(eng, cimg, bufs)
        rc = E.lib().mx_gemm_device_op(eng._ctx, int(fp32), int(beta), ta, tb,
                                       M, K, N, dA, lda, dB, ldb, dC,
                                       cimg.shape[0])
        if rc != 0:
            return {"ok": False, "rc": rc, "first_bad": None,
                    "sentinel_inside": False, "pad_ok": False, "cfg": None,
                    "loop": None, "op": None}
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        res = _exact._check_image(got, M, N, ref,
                                  sentinel.view(_exact.UINT[dt]))
        res["rc"] = 0
        res["cfg"] = eng.last_gemm_config()
        res["loop"] = eng.last_gemm_loop()
        res["op"] = list(eng.last_gemm_op())
        return res
    finally:
        for d in bufs:
            eng.free(d)


def _c_image(c, c0, dt):
    """C with ldc = M+16 and a trailing column: the NaN sentinel
    everywhere (beta 0), or C0 inside the finite sentinel (beta 1)."""
    nan = _exact._nan(dt)
    ldc = c.M + _exact.PAD
    if c.beta:
        sentinel = dt(_exact.FINITE_SENTINEL)
        return _exact._padded(c0, ldc, 1, sentinel), sentinel
    return _exact._filled(ldc, c.N + 1, nan), nan


def run_op_case(eng, c, ta, tb):
    """Case c as C (+)= op(A)·op(B): every pitch is dim+16, all A/B pad
    rows hold the NaN sentinel, C carries its sentinel plus a trailing
    column (the four conditions of _exact._check_image)."""
    dt = _exact.dtype_of(c.fp32)
    a, b, c0, ref = _exact.gemm_inputs(c)
    sa, sb = stored(a, ta), stored(b, tb)
    lda, ldb = sa.shape[0] + _exact.PAD, sb.shape[0] + _exact.PAD
    nan = _exact._nan(dt)
    cimg, sentinel = _c_image(c, c0, dt)
    return _run(eng, c.fp32, c.beta, ta, tb, c.M, c.K, c.N,
                _exact._padded(sa, lda, 0, nan), lda,
                _exact._padded(sb, ldb, 0, nan), ldb, cimg, ref, sentinel,
                alias=False)


def alias_inputs(fp32):
    """(S, ref): one stored K x M image S used in both roles, A^T·A with
    dA == dB: C = S^T·S, M = N = 384 (3 x 3 blocks), K = 48 (3 tiles).
    S is case (384, 256, 48)'s A^T, so the _exact bounds cover it."""
    m, k = ALIAS_SHAPE
    a = _exact.gemm_inputs(Case(fp32, 0, m, 256, k))[0]      # m x k
    s = np.asfortranarray(a.T)                               # k x m
    ref = a.astype(np.float64) @ a.astype(np.float64).T
    return s, ref


def run_alias_case(eng, fp32):
    dt = _exact.dtype_of(fp32)
    s, ref = alias_inputs(fp32)
    k, m = s.shape
    ld = k + _exact.PAD
    nan = _exact._nan(dt)
    cimg = _exact._filled(m + _exact.PAD, m + 1, nan)
    img = _exact._padded(s, ld, 0, nan)
    return _run(eng, fp32, 0, 1, 0, m, k, m, img, ld, None, ld, cimg, ref,
                nan, alias=True)
