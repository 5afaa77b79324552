# Componentwise rounding check of the GEMM family against a high-precision
# reference (shared by test_gpu_gemm_rounding.py, its child
# gemm_rounding_worker.py and the CPU-only test_rounding_cases.py). No GPU is
# needed to import this.
#
# The exact-integer tests prove indexing and the bit-identity tests tie the
# entries to each other; neither says anything about the arithmetic itself:
# a kernel that fed the MFMA operands cut to 10 mantissa bits, accumulated
# toward zero or flushed subnormals would pass them all. Here every result
# element is compared with R = op(A) op(B) (+ C0 | + addC) taken in a wider
# type from the SAME rounded inputs, on the scale of that element,
#
#     Sigma = |op(A)| |op(B)| (+ |C0| | + |addC|),
#     t_ij  = (C_ij - R_ij) / (u Sigma_ij),    u = 2^-24 (fp32), 2^-53 (fp64),
#
# and where Sigma_ij = 0 the result must be exactly 0.
#
# H, the hard bound (asserted on everything):
#     |C - R| <= gamma_terms Sigma + 2 terms eta + ref_err,
#     gamma_t = t u / (1 - t u)
# `terms` is the number of summands of an element. A sum of `terms` numbers
# formed from products takes at most `terms` roundings along any path from a
# product to the result, whatever the order, fused or not (Higham, Accuracy
# and Stability, section 3.1): that is gamma_terms Sigma. eta is half the
# smallest subnormal (2^-150 / 2^-1075): each of the at most 2 terms
# operations can also lose that much to gradual underflow. ref_err is the
# reference's own error: terms 2^-64 Sigma for np.longdouble, terms 2^-53
# Sigma for the float64 reference of fp32 (whose products are exact). No
# correct IEEE round-to-nearest kernel can exceed H; it is not a tuned number.
#
# H is loose by a factor of about `terms`. Two statistics see a rounding
# that is biased, or coarser than declared, inside it:
#   S1  classes pos and mix:  rms(t) <= sqrt(terms / 3)
#       (each rounding error is at most 1 in units of u Sigma and has
#       variance at most 1/3; they add at worst as independent terms)
#   S2  class pos:  |mean(t)| <= 8 sqrt(terms / 3) / sqrt(M N)
#       (eight standard errors of the mean of a zero-mean model)
# test_rounding_cases.py shows on the CPU that correct chains in three
# orders pass all three and that each degraded model below is rejected by
# the criterion meant for it.
#
# Data classes (all rounded to the element type before anything else sees
# them; the reference is taken from the rounded values):
#   pos      U[0, 1)
#   mix      U[0, 1) - 0.5: mixed sign, so sums cancel
#   wide     mix * 2^e, e an integer uniform in [-20, 20] per element: the
#            scale of an element must be right, not just the norm
#   sub_out  both operands mix * 2^-68 (fp32) / mix * 2^-520 (fp64): every
#            product and every result is subnormal
#   sub_in   A = mix * 2^-130 / 2^-1030 (subnormal inputs), B = mix * 2^40:
#            normal results
import functools
import math

import numpy as np

import _exact
import _exact_op
from _exact import PAD, UINT, _bits, _dev, _filled, _nan, _padded, dtype_of
from oracle import gen_matrix

assert np.finfo(np.longdouble).nmant >= 63, (
    "the fp64 rounding reference needs np.longdouble with a 64-bit "
    f"significand; this numpy gives {np.finfo(np.longdouble).nmant + 1} bits")

CLASSES = ("pos", "mix", "wide", "sub_out", "sub_in")
KS = (16, 64, 272, 1040)       # 1, 4, 17, 65 k-steps of 16
M = N = 128
SUB_SHIFT = {"sub_out": (-520, -68), "sub_in": (-1030, -130)}   # (fp64, fp32)
SUB_IN_B_SHIFT = 40
S1_CLASSES = ("pos", "mix")
S2_CLASSES = ("pos",)
FORMS = dict(nn=(0, 0), **_exact_op.FORMS)


def ref_type(fp32):
    return np.float64 if fp32 else np.longdouble


def unit(fp32):
    """Unit roundoff of the element type."""
    return 2.0 ** (-24 if fp32 else -53)


def ref_unit(fp32):
    return 2.0 ** (-53 if fp32 else -64)


def eta(fp32):
    """Half the smallest subnormal, in the reference type (2^-1075 is not
    a float64)."""
    return np.ldexp(ref_type(fp32)(1), -150 if fp32 else -1075)


def tiny(fp32):
    """The smallest normal number of the element type."""
    return np.finfo(dtype_of(fp32)).tiny


def gamma(terms, u):
    return terms * u / (1 - terms * u)


# ---------------------------------------------------------------------------
# data
_ROLE = {"a": 1, "b": 2, "c": 3, "x": 4}


def _seed(cls, role, fp32, rows, cols, tag):
    s = 0x20C5
    for v in (CLASSES.index(cls), _ROLE[role], int(fp32), rows, cols, tag):
        s = (s * 1000003 + v + 1) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=None)
def operand(cls, role, fp32, rows, cols, tag=0):
    """rows x cols col-major matrix of class cls in the element type,
    read-only. role: "a" / "b" the operands, "c" an addend (C0 or addC),
    "x" a vector; tag tells apart operands of one shape."""
    dt = dtype_of(fp32)
    seed = _seed(cls, role, fp32, rows, cols, tag)
    g = gen_matrix(rows, cols, seed=seed)              # float64, U[0, 1)
    if cls == "pos":
        v = g
    elif cls == "mix":
        v = g - 0.5
    elif cls == "wide":
        e = np.random.RandomState(seed).randint(-20, 21, size=(rows, cols))
        v = np.ldexp(g - 0.5, e)
    else:
        assert role in "abx", "the subnormal classes have no addend"
        shift = SUB_SHIFT[cls][int(bool(fp32))]
        if cls == "sub_in" and role != "a":
            shift = SUB_IN_B_SHIFT
        v = np.ldexp(g - 0.5, shift)
    out = np.asfortranarray(v.astype(dt))              # rounded once, here
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def product(cls, fp32, m, k, n, tag=0):
    """(A m x k, B k x n, R, Sigma): the operands in the element type and
    R = A B, Sigma = |A| |B| in the reference type. Computed once per
    (class, type, shape, tag) and never modified."""
    rt = ref_type(fp32)
    a = operand(cls, "a", fp32, m, k, tag)
    b = operand(cls, "b", fp32, k, n, tag)
    al, bl = a.astype(rt), b.astype(rt)
    r, s = al @ bl, np.abs(al) @ np.abs(bl)
    for v in (r, s):
        v.setflags(write=False)
    return a, b, r, s


def with_addend(r, s, c, fp32):
    """(R + c, Sigma + |c|) for an addend c of the element type."""
    cl = c.astype(ref_type(fp32))
    return r + cl, s + np.abs(cl)


# ---------------------------------------------------------------------------
# the checker
def hard_bound(s, fp32, terms):
    """H's right-hand side, per element, in the reference type."""
    rt = ref_type(fp32)
    return ((rt(gamma(terms, unit(fp32))) + rt(terms * ref_unit(fp32))) * s
            + 2 * terms * eta(fp32))


def measure(got, r, s, fp32, terms):
    """The figures of one result `got` (element type) against (R, Sigma):
        bad        elements violating H (a NaN or inf result is one)
        first_bad  [row, col] of the first, or None
        h          max |C - R| / H's right-hand side (inf if not finite)
        zero_ok    C is exactly 0 wherever Sigma is 0
        rms, mean, tmax  of t (tmax of |t|) where Sigma > 0
        s1_limit, s2_limit  the limits of S1 and S2 for this case."""
    rt = ref_type(fp32)
    assert got.shape == r.shape == s.shape and got.dtype == dtype_of(fp32)
    with np.errstate(invalid="ignore", over="ignore"):
        err = got.astype(rt) - r
        ratio = np.abs(err) / hard_bound(s, fp32, terms)
        bad = ~(ratio <= 1)
        nz = s > 0
        t = err[nz] / (rt(unit(fp32)) * s[nz])
        hmax = ratio.max() if np.isfinite(ratio).all() else np.inf
        rms = np.sqrt(np.mean(t * t)) if t.size else rt(0)
        mean = np.mean(t) if t.size else rt(0)
        tmax = np.abs(t).max() if t.size else rt(0)
    where = np.argwhere(bad)
    sd = math.sqrt(terms / 3.0)
    with np.errstate(over="ignore"):
        return {
            "bad": int(bad.sum()),
            "first_bad": [int(v) for v in where[0]] if len(where) else None,
            "h": float(hmax),
            "zero_ok": bool((got[~nz] == 0).all()),
            "rms": float(rms), "mean": float(mean), "tmax": float(tmax),
            "terms": int(terms),
            "s1_limit": sd, "s2_limit": 8 * sd / math.sqrt(got.size),
        }


def criteria(cls):
    """The criteria a result of class cls is held to."""
    return (("H",) + (("S1",) if cls in S1_CLASSES else ())
            + (("S2",) if cls in S2_CLASSES else ()))


def failures(mes, which):
    """The criteria of `which` that the figures `mes` miss, with the
    figures, as a list of strings (empty: accepted)."""
    out = []
    if "H" in which and (mes["bad"] or not mes["zero_ok"]):
        out.append(f"H: {mes['bad']} elements over the bound, first at "
                   f"{mes['first_bad']}, max ratio {mes['h']:.3g}, "
                   f"zero_ok {mes['zero_ok']} (terms {mes['terms']})")
    if "S1" in which and not mes["rms"] <= mes["s1_limit"]:
        out.append(f"S1: rms t {mes['rms']:.4g} > {mes['s1_limit']:.4g}")
    if "S2" in which and not abs(mes["mean"]) <= mes["s2_limit"]:
        out.append(f"S2: |mean t| {abs(mes['mean']):.4g} > "
                   f"{mes['s2_limit']:.4g}")
    return out


def report_line(entry, fp32, k, cls, mes, note=""):
    """One line of figures, printed by the GPU test ahead of its
    assertions (profiles/gemm_rounding.md is made from these)."""
    g = mes["tmax"] * unit(fp32) / gamma(mes["terms"], unit(fp32))
    return (f"ROUNDING entry={entry} type={'f32' if fp32 else 'f64'} k={k} "
            f"class={cls} terms={mes['terms']} h={mes['h']:.4g} "
            f"max_t_over_gamma={g:.4g} rms_t={mes['rms']:.4g} "
            f"mean_t={mes['mean']:+.4g} bad={mes['bad']}"
            + (f" {note}" if note else ""))


# ---------------------------------------------------------------------------
# numpy chains: three correct orders, and the degraded models
def _start(a, b, c0):
    dt = a.dtype.type
    if c0 is None:
        return np.zeros((a.shape[0], b.shape[1]), dtype=dt)
    return np.array(c0, dtype=dt)


def chain_sequential(a, b, c0=None):
    """Ascending k, product and sum each rounded to nearest in the
    element type."""
    acc = _start(a, b, c0)
    for l in range(a.shape[1]):
        acc = acc + a[:, l:l + 1] * b[l:l + 1, :]
    return acc


def chain_group4(a, b, c0=None):
    """Four products added to the accumulator in the reference type, one
    rounding per group of four k."""
    fp32 = a.dtype == np.float32
    rt, dt = ref_type(fp32), a.dtype.type
    acc = _start(a, b, c0)
    for l in range(0, a.shape[1], 4):
        acc = (acc.astype(rt)
               + a[:, l:l + 4].astype(rt) @ b[l:l + 4, :].astype(rt)).astype(dt)
    return acc


def chain_pairwise(a, b, c0=None):
    """Rounded products summed as a balanced binary tree, the addend last."""
    def tree(lo, hi):
        if hi - lo == 1:
            return a[:, lo:hi] * b[lo:hi, :]
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)
    out = tree(0, a.shape[1])
    return out if c0 is None else out + c0


def cut_mantissa(x, keep):
    """x with its stored mantissa cut (toward zero) to `keep` bits."""
    nmant = np.finfo(x.dtype).nmant
    ut = UINT[x.dtype.type]
    mask = ut(~((1 << (nmant - keep)) - 1) & ((1 << (8 * x.itemsize)) - 1))
    return (np.ascontiguousarray(x).view(ut) & mask).view(x.dtype)


def chain_toward_zero(a, b, c0=None):
    """Model (c): ascending k, each accumulate rounded toward zero."""
    fp32 = a.dtype == np.float32
    rt, dt = ref_type(fp32), a.dtype.type
    acc = _start(a, b, c0)
    for l in range(a.shape[1]):
        s = acc.astype(rt) + a[:, l:l + 1].astype(rt) * b[l:l + 1, :].astype(rt)
        r = s.astype(dt)
        over = np.abs(r.astype(rt)) > np.abs(s)
        r[over] = np.nextafter(r[over], dt(0))
        acc = r
    return acc


def flush_subnormal(x):
    """Model (d): every subnormal of x replaced by zero."""
    out = np.array(x)
    out[np.abs(out) < np.finfo(x.dtype).tiny] = 0
    return out


def move_one(r, s, fp32, terms, at):
    """Model (e): R rounded to the element type, with the element `at`
    moved by (terms + 2) u Sigma, away from R."""
    rt, dt = ref_type(fp32), dtype_of(fp32)
    out = r.astype(dt)
    sign = -1 if out[at].astype(rt) < r[at] else 1
    out[at] = dt(r[at] + sign * rt((terms + 2) * unit(fp32)) * s[at])
    return out


# ---------------------------------------------------------------------------
# device runs (images and conventions of tests/_exact.py: pitches larger
# than the dims, NaN in every pad of A and B, C prefilled with the NaN
# sentinel, or C0 inside the finite sentinel when accumulating, plus one
# guard column)
def _c_image(fp32, c0, m, n):
    dt = dtype_of(fp32)
    ldc = m + PAD
    if c0 is not None:
        sentinel = dt(_exact.FINITE_SENTINEL)
        return _padded(np.asfortranarray(c0), ldc, 1, sentinel), sentinel
    return _filled(ldc, n + 1, _nan(dt)), _nan(dt)


def split_c(img, rows, cols, sentinel):
    """(interior copy, pad rows and guard column untouched, sentinel found
    inside) of a downloaded C image."""
    sb = sentinel.view(UINT[img.dtype.type])
    inner = np.array(img[:rows, :cols], order="F")
    pad_ok = bool((_bits(img[rows:, :]) == sb).all()
                  and (_bits(img[:, cols:]) == sb).all())
    return inner, pad_ok, bool((_bits(inner) == sb).any())


def _fail(rc):
    return {"rc": rc, "got": None}


def run_op(eng, fp32, form, a, b, c0=None, slices=None):
    """C (+)= op(A) op(B) for logical A (m x k), B (k x n) through
    mx_gemm_device_op, or mx_gemm_device_splitk where slices is given.
    Returns {"rc", "got", "pad_ok", "sentinel_inside", "cfg", "loop",
    "op", "splitk"}."""
    from marlin_amd import engine as E
    ta, tb = FORMS[form]
    dt = dtype_of(fp32)
    nan = _nan(dt)
    (m, k), n = a.shape, b.shape[1]
    sa, sb = _exact_op.stored(a, ta), _exact_op.stored(b, tb)
    lda, ldb = sa.shape[0] + PAD, sb.shape[0] + PAD
    cimg, sentinel = _c_image(fp32, c0, m, n)
    beta = int(c0 is not None)
    bufs = []
    try:
        dA = _dev(eng, _padded(sa, lda, 0, nan), bufs)
        dB = _dev(eng, _padded(sb, ldb, 0, nan), bufs)
        dC = _dev(eng, cimg, bufs)
        if slices is None:
            rc = E.lib().mx_gemm_device_op(eng._ctx, int(fp32), beta, ta, tb,
                                           m, k, n, dA, lda, dB, ldb, dC,
                                           cimg.shape[0])
        else:
            rc = eng.gemm_splitk_raw(m, k, n, dA, lda, dB, ldb, dC,
                                     cimg.shape[0], slices, fp32, beta, ta,
                                     tb, check=False)
        if rc != 0:
            return _fail(rc)
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        inner, pad_ok, inside = split_c(got, m, n, sentinel)
        return {"rc": 0, "got": inner, "pad_ok": pad_ok,
                "sentinel_inside": inside, "cfg": eng.last_gemm_config(),
                "loop": eng.last_gemm_loop(), "op": list(eng.last_gemm_op()),
                "splitk": (list(eng.last_gemm_splitk())
                           if slices is not None else None)}
    finally:
        for d in bufs:
            eng.free(d)


def run_epilogue(eng, a, b, add=None):
    """C[n x m] = (A B)^T (+ addC) through mx_sgemm_epilogue_device (fp32):
    lda = m + 16, ldb = k + 16, ldc = n + 16, addC's pads NaN."""
    from marlin_amd import engine as E
    dt = np.float32
    nan = _nan(dt)
    (m, k), n = a.shape, b.shape[1]
    lda, ldb, ldc = m + PAD, k + PAD, n + PAD
    cimg = _filled(ldc, m + 1, nan)
    bufs = []
    try:
        dA = _dev(eng, _padded(a, lda, 0, nan), bufs)
        dB = _dev(eng, _padded(b, ldb, 0, nan), bufs)
        dC = _dev(eng, cimg, bufs)
        dAdd = (_dev(eng, _padded(np.asfortranarray(add), ldc, 1, nan), bufs)
                if add is not None else None)
        rc = E.lib().mx_sgemm_epilogue_device(eng._ctx, m, k, n, dA, lda, dB,
                                              ldb, dC, ldc, dAdd)
        if rc != 0:
            return _fail(rc)
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        inner, pad_ok, inside = split_c(got, n, m, nan)
        return {"rc": 0, "got": inner, "pad_ok": pad_ok,
                "sentinel_inside": inside}
    finally:
        for d in bufs:
            eng.free(d)


def run_grouped(eng, fp32, pairs):
    """[(A, B)] as one mx_gemm_device_grouped call (NN, beta 0). Returns
    {"rc", "group", "problems": [the records of run_op]}."""
    dt = dtype_of(fp32)
    nan = _nan(dt)
    bufs, rows, imgs = [], [], []
    try:
        for a, b in pairs:
            (m, k), n = a.shape, b.shape[1]
            cimg, sentinel = _c_image(fp32, None, m, n)
            dA = _dev(eng, _padded(a, m + PAD, 0, nan), bufs)
            dB = _dev(eng, _padded(b, k + PAD, 0, nan), bufs)
            dC = _dev(eng, cimg, bufs)
            rows.append((m, k, n, dA, 0, m + PAD, dB, 0, k + PAD, dC, 0,
                         cimg.shape[0]))
            imgs.append((dC, cimg, m, n, sentinel))
        rc = eng.gemm_grouped_raw(rows, fp32, check=False)
        if rc != 0:
            return {"rc": rc, "problems": []}
        out = {"rc": 0, "group": list(eng.last_gemm_group()), "problems": []}
        for dC, cimg, m, n, sentinel in imgs:
            got = np.empty_like(cimg)
            eng.download(got, dC, got.nbytes)
            inner, pad_ok, inside = split_c(got, m, n, sentinel)
            out["problems"].append({"rc": 0, "got": inner, "pad_ok": pad_ok,
                                    "sentinel_inside": inside})
        return out
    finally:
        for d in bufs:
            eng.free(d)


def run_summa_position(eng, fp32, pr, pc, prow, pcol, a, b, kb):
    """Position (prow, pcol) of a pr x pc grid through
    mx_gemm_summa_virtual on the shards of the global A (m x k), B (k x n),
    built by tests/_exact_summa.py. Returns {"rc", "got" (this position's
    block), "rows", "cols" (its slice of C), "pad_ok", "sentinel_inside",
    "pad_rows_zero", "pad_cols_zero", "launches", "panels"}."""
    import _exact_summa as XS
    from marlin_amd import engine as E
    from marlin_amd.engine import EngineError
    dt = dtype_of(fp32)
    (m, k), n = a.shape, b.shape[1]
    c = XS.SummaCase(int(fp32), pr, pc, m, k, n, kb)
    g = XS.Geometry(c, prow, pcol)
    assert not g.empty
    cimg = XS.c_image(c, g)
    bufs = []
    try:
        dA = [XS._upload(eng, XS.a_shard(c, prow, j, a), bufs)
              for j in range(pc)]
        dB = [XS._upload(eng, XS.b_shard(c, i, pcol, b), bufs)
              for i in range(pr)]
        dC = _dev(eng, cimg, bufs)
        try:
            eng.gemm_summa_virtual(pr, pc, prow, pcol, m, k, n, dA, dB, dC,
                                   kb, bool(fp32))
        except EngineError as e:
            return _fail(e.code)
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        sb = _nan(dt).view(UINT[dt])
        inner = np.array(got[:g.mi, :g.nj], order="F")
        return {"rc": 0, "got": inner,
                "rows": (g.mo, g.mo + g.mi), "cols": (g.no, g.no + g.nj),
                "pad_ok": bool((_bits(got[:, g.njp:]) == sb).all()),
                "sentinel_inside": bool((_bits(inner) == sb).any()),
                "pad_rows_zero": bool((got[g.mi:, :g.njp] == 0).all()),
                "pad_cols_zero": bool((got[:, g.nj:g.njp] == 0).all()),
                "launches": int(eng.stats()["gemm_launches"]),
                "panels": len(E.plan_panels(k, pr, pc, kb))}
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# the latched variants (one fresh child process each: gemm_rounding_worker.py)
KNOBS = ("MARLIN_GEMM_CFG", "MARLIN_GEMM_REMAP", "MARLIN_GEMM_BAND",
         "MARLIN_GEMM_PHASE", "MARLIN_GEMM_LOOP")
VARIANTS = {
    "bk32": {"MARLIN_GEMM_CFG": "bk32"},
    "bm256": {"MARLIN_GEMM_CFG": "bm256"},
    "twobar": {"MARLIN_GEMM_LOOP": "twobar"},
    "pipe": {"MARLIN_GEMM_LOOP": "pipe"},
}
_VARIANT_CLASSES = ("pos", "mix", "sub_out")


def variant_cases(variant):
    """[(fp32, beta, cls, m, n, k)] a variant's child runs. sub_out runs
    at the shortest k only and never accumulates (it has no addend)."""
    if variant == "bk32":
        types, m, ks = (0, 1), M, (32, 288, 1056)
    elif variant == "bm256":
        types, m, ks = (0,), 256, (16, 272)
    else:
        types, m, ks = (0, 1), M, (16, 64, 272)
    out = []
    for fp32 in types:
        for cls in _VARIANT_CLASSES:
            for k in (ks[:1] if cls == "sub_out" else ks):
                out.append((fp32, 0, cls, m, N, k))
            if cls != "sub_out":
                out.append((fp32, 1, cls, m, N, ks[1]))
    return out


def variant_case_id(case):
    fp32, beta, cls, m, n, k = case
    return f"{'f32' if fp32 else 'f64'}-b{beta}-{cls}-{m}x{n}x{k}"


def variant_expected(variant, fp32):
    """(bk, bm, loop) the variant must report for its cases. The default
    loop is pipelined for every variant but fp32 at bk 16."""
    bk = 32 if variant == "bk32" else 16
    bm = 256 if variant == "bm256" else 128
    if variant in ("twobar", "pipe"):
        loop = int(variant == "pipe")
    else:
        loop = 0 if (fp32 and bk == 16) else 1
    return bk, bm, loop


def case_inputs(case):
    """(A, B, C0 or None) of a variant case (no reference is computed)."""
    fp32, beta, cls, m, n, k = case
    return (operand(cls, "a", fp32, m, k), operand(cls, "b", fp32, k, n),
            operand(cls, "c", fp32, m, n) if beta else None)


def case_reference(case):
    """(R, Sigma, terms) of a variant case."""
    fp32, beta, cls, m, n, k = case
    _, _, r, s = product(cls, fp32, m, k, n)
    if beta:
        r, s = with_addend(r, s, operand(cls, "c", fp32, m, n), fp32)
    return r, s, k + beta
