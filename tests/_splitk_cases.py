# Cases of the split-K GEMM entry (mx_gemm_device_splitk), shared by
# test_gpu_gemm_splitk.py, its child gemm_splitk_worker.py and the CPU-only
# test_gemm_splitk_plan.py. Two kinds of data:
#   exact   tests/_exact.py's small integers, on which every product and
#           every partial sum in ANY order is representable, so the split
#           result is compared with assert_array_equal against the exact
#           product whatever S is;
#   fold    ordinary rounding data (gen_matrix - 0.5: mixed sign, no
#           denormals), on which the result DOES depend on the order: the
#           entry's spec, a left fold in the element type of the plain
#           entry's per-slice products, is rebuilt in numpy and compared
#           bit for bit.
# Also the Python restatement of the slicing policy of
# marlin_amd/csrc/gemm_splitk_plan.h (test_gemm_splitk_plan.py compares the
# two on the CPU over the header's whole sweep).
import hashlib
import os
import re

import numpy as np

import _exact
import _exact_op
from _exact import Case

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), "marlin_amd", "csrc",
                      "gemm_splitk_plan.h")

FORMS = dict(nn=(0, 0), **_exact_op.FORMS)
LOOPS = {"twobar": {"MARLIN_GEMM_LOOP": "twobar"},
         "pipe": {"MARLIN_GEMM_LOOP": "pipe"}}
KNOBS = ("MARLIN_GEMM_CFG", "MARLIN_GEMM_REMAP", "MARLIN_GEMM_BAND",
         "MARLIN_GEMM_PHASE", "MARLIN_GEMM_LOOP")


# ---------------------------------------------------------------------------
# the policy, restated
def _constant(name):
    m = re.search(rf"constexpr int64_t {name} = (\d+);", open(HEADER).read())
    return int(m.group(1))


def min_ksteps():
    """MX_SPLITK_MIN_KSTEPS as the header states it (a measured constant:
    read, never asserted)."""
    return _constant("MX_SPLITK_MIN_KSTEPS")


def fill_div():
    """MX_SPLITK_FILL_DIV, the other measured constant."""
    return _constant("MX_SPLITK_FILL_DIV")


def resident(fp32, cus):
    return max(cus, 0) * (4 if fp32 else 2)


def auto_slices(fp32, m, n, k, cus):
    tiles = (m // 128) * (n // 128)
    target = resident(fp32, cus) // fill_div()
    if tiles <= 0 or k <= 0 or tiles >= target:
        return 1
    return max(1, min(target // tiles, (k // 16) // min_ksteps()))


def slices(k, s):
    """[(start, len)] in k-steps of 16: s clamped to [1, k / 16], lengths
    as even as possible, the longer ones first."""
    steps = max(k, 0) // 16
    s = max(1, min(max(s, 1), steps))
    base, longer = divmod(steps, s)
    out, at = [], 0
    for i in range(s):
        ln = base + (1 if i < longer else 0)
        out.append((at, ln))
        at += ln
    return out


# ---------------------------------------------------------------------------
# 1. exact integers. (m, n, k, S asked, S effective): one step per slice
# (every slice is only the peeled last k-step), the same with three, an
# uneven 3 / 2 / 2 split over 2 x 3 blocks, and a count clamped to k / 16.
EXACT_SHAPES = [(128, 128, 32, 2, 2), (128, 128, 48, 3, 3),
                (256, 384, 112, 3, 3), (128, 256, 48, 8, 3)]
COMBOS = [(fp32, beta, form) for fp32 in (0, 1) for beta in (0, 1)
          for form in FORMS]


def combo_id(fp32, beta, form):
    return f"{'f32' if fp32 else 'f64'}-b{beta}-{form}"


def shape_id(shape):
    m, n, k, s, _ = shape
    return f"{m}x{n}x{k}-S{s}"


def run_exact(eng, fp32, beta, form, m, n, k, s):
    """Case (m, n, k) as C (+)= op(A)·op(B) through the split-K entry with
    `s` slices: every pitch is dim + PAD, A / B pad rows hold NaN, C carries
    its sentinel in the pad rows and one guard column. Returns
    _exact._check_image's record plus rc, splitk, group, op, stats."""
    ta, tb = FORMS[form]
    dt = _exact.dtype_of(fp32)
    nan = _exact._nan(dt)
    c = Case(fp32, beta, m, n, k)
    a, b, c0, ref = _exact.gemm_inputs(c)
    sa, sb = _exact_op.stored(a, ta), _exact_op.stored(b, tb)
    lda, ldb = sa.shape[0] + _exact.PAD, sb.shape[0] + _exact.PAD
    cimg, sentinel = _exact_op._c_image(c, c0, dt)
    bufs = []
    try:
        dA = _exact._dev(eng, _exact._padded(sa, lda, 0, nan), bufs)
        dB = _exact._dev(eng, _exact._padded(sb, ldb, 0, nan), bufs)
        dC = _exact._dev(eng, cimg, bufs)
        rc = eng.gemm_splitk_raw(m, k, n, dA, lda, dB, ldb, dC, cimg.shape[0],
                                 s, fp32, beta, ta, tb, check=False)
        if rc != 0:
            return {"rc": rc}
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        res = _exact._check_image(got, m, n, ref,
                                  sentinel.view(_exact.UINT[dt]))
        st = eng.stats()
        res.update(rc=0, splitk=list(eng.last_gemm_splitk()),
                   group=list(eng.last_gemm_group()),
                   op=list(eng.last_gemm_op()), launches=st["gemm_launches"],
                   flops=st["flops"], cfg=eng.last_gemm_config())
        return res
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# 2. the fold spec on rounding data: 2 x 1 blocks, 5 k-steps
FOLD_M, FOLD_N, FOLD_K = 256, 128, 80
FOLD_CASES = [(fp32, form, s, beta) for fp32 in (0, 1)
              for form in ("nn", "tn") for s in (2, 5) for beta in (0, 1)]


def fold_id(fp32, form, s, beta):
    return f"{'f32' if fp32 else 'f64'}-{form}-S{s}-b{beta}"


def fold_inputs(fp32):
    """(A m x k, B k x n, C0 m x n), entries in [-0.5, 0.5)."""
    from oracle import gen_matrix
    dt = _exact.dtype_of(fp32)

    def g(r, c, seed):
        return np.asfortranarray(
            (gen_matrix(r, c, seed=seed, dtype=dt) - dt(0.5)).astype(dt))
    return (g(FOLD_M, FOLD_K, 0x5A00 + fp32), g(FOLD_K, FOLD_N, 0x5B00 + fp32),
            g(FOLD_M, FOLD_N, 0x5C00 + fp32))


def _plain(eng, fp32, beta, ta, tb, m, k, n, dA, lda, dB, ldb, dC, ldc):
    from marlin_amd import engine as E
    return E.lib().mx_gemm_device_op(eng._ctx, fp32, beta, ta, tb, m, k, n,
                                     dA, lda, dB, ldb, dC, ldc)


def _fetch(eng, d, like):
    got = np.empty_like(like)
    eng.download(got, d, got.nbytes)
    return got


def run_fold(eng, fp32, form, s, beta):
    """{"rc", "equal", "real", "digest", "splitk", "group"}: the split-K
    result against the numpy left fold of the plain entry's products of
    each k-slice, uploaded as matrices of their own. digest is the sha256
    of the split result's bytes (the loop children are compared by it)."""
    ta, tb = FORMS[form]
    dt = _exact.dtype_of(fp32)
    U = _exact.UINT[dt]
    a, b, c0 = fold_inputs(fp32)
    m, n, k = FOLD_M, FOLD_N, FOLD_K
    sa, sb = _exact_op.stored(a, ta), _exact_op.stored(b, tb)
    bufs = []
    try:
        dA, dB = _exact._dev(eng, sa, bufs), _exact._dev(eng, sb, bufs)
        dC = _exact._dev(eng, c0, bufs)
        rc = eng.gemm_splitk_raw(m, k, n, dA, sa.shape[0], dB, sb.shape[0],
                                 dC, m, s, fp32, beta, ta, tb, check=False)
        if rc != 0:
            return {"rc": rc}
        got = _fetch(eng, dC, c0)
        splitk, group = eng.last_gemm_splitk(), eng.last_gemm_group()
        parts = []
        for start, ln in slices(k, s):
            ks = slice(16 * start, 16 * (start + ln))
            pa = _exact_op.stored(np.asfortranarray(a[:, ks]), ta)
            pb = _exact_op.stored(np.asfortranarray(b[ks, :]), tb)
            dPa, dPb = _exact._dev(eng, pa, bufs), _exact._dev(eng, pb, bufs)
            dP = _exact._dev(eng, _exact._filled(m, n, _exact._nan(dt)), bufs)
            rc = _plain(eng, fp32, 0, ta, tb, m, 16 * ln, n, dPa, pa.shape[0],
                        dPb, pb.shape[0], dP, m)
            if rc != 0:
                return {"rc": rc}
            parts.append(_fetch(eng, dP, c0))
        acc = c0.copy() if beta else parts.pop(0)
        for p in parts:
            acc = (acc + p).astype(dt)          # one rounding per add, in dt
        # the data does round: the unsplit product has other bits
        dU = _exact._dev(eng, c0, bufs)
        rc = _plain(eng, fp32, beta, ta, tb, m, k, n, dA, sa.shape[0], dB,
                    sb.shape[0], dU, m)
        if rc != 0:
            return {"rc": rc}
        unsplit = _fetch(eng, dU, c0)
        return {"rc": 0,
                "equal": bool((got.view(U) == acc.view(U)).all()),
                "real": bool(np.isfinite(got).all()
                             and (got.view(U) != unsplit.view(U)).any()
                             and np.allclose(got, unsplit, rtol=0,
                                             atol=1e-3 if fp32 else 1e-12)),
                "digest": hashlib.sha256(got.tobytes()).hexdigest(),
                "splitk": list(splitk), "group": list(group),
                "loop": eng.last_gemm_loop()}
    finally:
        for d in bufs:
            eng.free(d)
