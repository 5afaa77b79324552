# Shapes, inputs and device runs of the triangular-solve tests
# (test_gpu_trsm.py, test_gpu_trsm_consumers.py) and the Python restatement
# of the entry's argument check that test_trsm_plan.py compares with the
# C++ (marlin_amd/csrc/trsm_plan.h), and the numpy restatement of the
# diagonal kernel's arithmetic (stage_restated, substitute_restated) that
# test_gpu_diag_bits.py compares the device with on rounding data. No GPU is
# needed to import this.
#
# Exact data: X is integer in [-8, 8]; T has off-diagonal integers in
# [-2, 2] and a diagonal from {+-1/2, +-1, +-2, +-4} (1 when unit_diag);
# B = op(T) X (or X op(T)) is formed in float64, where it is exact. Every
# intermediate of a substitution in any blocked order is then x_i times a
# power of two, or a partial sum of |t| |x| terms and one b: a multiple of
# 1/2 below 2 * (300 * 16 + 32) < 2^14, exact in fp32 and fp64 alike, and a
# quotient is (t_ii x_i) / t_ii. A correct solve returns X bit for bit, but
# for the sign of a zero: where x_i = 0 the numerator is an exact zero of
# either sign, which a negative t_ii turns over (any substitution does, a
# BLAS one too), so X is compared as numbers, under which -0 == +0 and
# nothing else differs from a comparison of bits on finite data.
import functools
import itertools

import numpy as np

import _exact
from _exact import PAD, UINT, _dev, _filled, _nan, dtype_of

EINVAL = -4
W = 128

# (side, lower, trans, unit_diag): all 16
FORMS = list(itertools.product((0, 1), repeat=4))
ORDERS = [1, 127, 128, 129, 300]
RHS = [128, 256]
DIAG = np.array([0.5, -0.5, 1, -1, 2, -2, 4, -4])


def form_id(f):
    side, lower, trans, unit = f
    return ("RL"[1 - side] + "UL"[lower] + "NT"[trans] + "NU"[unit])


def r128(x):
    return (x + W - 1) // W * W


# ---------------------------------------------------------------------------
# the argument check, restated (aliasing aside: it needs device pointers)
def check(w, fp32, side, lower, trans, unit, n, r, bytes_t, ldt, bytes_b, ldb):
    """(rc, empty) of mx_trsm_check for two distinct, disjoint buffers of
    the given sizes. Python integers: nothing can overflow."""
    if any(f not in (0, 1) for f in (fp32, side, lower, trans, unit)):
        return EINVAL, False
    if n < 0 or r < 0 or r % w:
        return EINVAL, False
    if n == 0 or r == 0:
        return 0, True
    np_ = (n + w - 1) // w * w
    if np_ > 2 ** 63 - 1:
        return EINVAL, False
    elem = 4 if fp32 else 8
    e16 = 16 // elem
    brows, bcols = (r, np_) if side else (np_, r)
    if ldt < np_ or ldb < brows or ldt % e16 or ldb % e16:
        return EINVAL, False
    if (np_ - 1) * ldt + np_ > bytes_t // elem:
        return EINVAL, False
    if (bcols - 1) * ldb + brows > bytes_b // elem:
        return EINVAL, False
    if (np_ // w) * (r // w) > 2 ** 31 - 1 or 2 * (r // w) > 2 ** 31 - 1:
        return EINVAL, False
    return 0, False


def sweep_forward(side, lower, trans):
    """The direction of the blocked sweep (include/marlin_gpu.h)."""
    eff_lower = lower ^ trans
    return bool(eff_lower) if side == 0 else not eff_lower


# ---------------------------------------------------------------------------
# inputs
def _seed(*key):
    s = 0x7A5E
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return s


def triangle_mask(n, lower):
    i, j = np.indices((n, n))
    return i >= j if lower else i <= j


@functools.lru_cache(maxsize=None)
def exact_problem(side, lower, trans, unit, n, r):
    """(T, X, B) in float64, exact: T n x n with zeros outside its triangle,
    X and B n x r (left) or r x n (right). Never modified."""
    rng = np.random.RandomState(_seed(side, lower, trans, unit, n, r))
    t = rng.randint(-2, 3, size=(n, n)).astype(np.float64)
    t *= triangle_mask(n, lower)
    d = np.ones(n) if unit else DIAG[rng.randint(0, 8, size=n)]
    t[np.arange(n), np.arange(n)] = d
    x = rng.randint(-8, 9, size=(r, n) if side else (n, r)).astype(np.float64)
    op = t.T if trans else t
    b = x @ op if side else op @ x
    out = tuple(np.asfortranarray(v) for v in (t, x, b))
    for v in out:
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rounding_problem(fp32, side, lower, trans, n, r):
    """(T, B) in the element type: T uniform in [-1, 1] off the diagonal,
    2 + U[0, 1) on it, zeros outside its triangle; B uniform in [-1, 1]."""
    dt = dtype_of(fp32)
    rng = np.random.RandomState(_seed(9, fp32, side, lower, trans, n, r))
    t = rng.uniform(-1, 1, size=(n, n)) * triangle_mask(n, lower)
    t[np.arange(n), np.arange(n)] = 2 + rng.uniform(0, 1, size=n)
    b = rng.uniform(-1, 1, size=(r, n) if side else (n, r))
    out = (np.asfortranarray(t.astype(dt)), np.asfortranarray(b.astype(dt)))
    for v in out:
        v.setflags(write=False)
    return out


def t_image(t, lower, unit, ldt, dt, poison=True):
    """The device image of T: np x np at pitch ldt. With poison, NaN sits
    wherever the contract says nothing is read: the opposite triangle, a
    unit diagonal, the last diagonal block at an index >= n, the pitch pad.
    The part of the referenced off-diagonal blocks at an index >= n is
    zero, as the contract asks."""
    n = t.shape[0]
    np_ = r128(n)
    img = _filled(ldt, np_, _nan(dt)) if poison else np.zeros(
        (ldt, np_), dtype=dt, order="F")
    i, j = np.indices((np_, np_))
    ref = (i >= j) if lower else (i <= j)
    last = np_ - W
    pad = ((i >= n) | (j >= n)) & ref & ~((i >= last) & (j >= last))
    img[:np_, :][pad] = 0
    inside = ref[:n, :n].copy()
    if unit:
        inside[np.arange(n), np.arange(n)] = False
    img[:n, :n][inside] = t.astype(dt)[inside]
    return img


def b_image(b, side, n, r, ldb, dt, poison=True):
    """The device image of B with one guard column behind it: the logical
    part, zeros in the pad [n, np), and (poison) NaN in the pitch pad and
    the guard column."""
    np_ = r128(n)
    cols = (np_ if side else r) + 1
    img = _filled(ldb, cols, _nan(dt)) if poison else np.zeros(
        (ldb, cols), dtype=dt, order="F")
    if side:
        img[:r, :np_] = 0
        img[:r, :n] = b
    else:
        img[:np_, :r] = 0
        img[:n, :r] = b
    return img


def split_b_image(img, side, n, r):
    """(logical part, pad [n, np), mask of the sentinel positions)."""
    np_ = r128(n)
    sent = np.ones(img.shape, dtype=bool)
    if side:
        sent[:r, :np_] = False
        return img[:r, :n], img[:r, n:np_], sent
    sent[:np_, :r] = False
    return img[:n, :r], img[n:np_, :r], sent


def zero_sign_dropped(x):
    """x with every -0 replaced by +0 and no other bit changed: the one
    normalisation under which the exact results are compared bit for bit."""
    out = np.array(x, copy=True, order="F")
    out[out == 0] = 0
    return out


def fetch(eng, d, like):
    got = np.empty_like(like)
    eng.download(got, d, got.nbytes)
    return got


def solve_images(eng, fp32, form, n, r, timg, bimg, repeat=1):
    """Upload both images, run the entry `repeat` times from the same B,
    return (rc, [B image after each run], stats, T image after)."""
    side, lower, trans, unit = form
    bufs, outs = [], []
    try:
        dT = _dev(eng, timg, bufs)
        dB = _dev(eng, bimg, bufs)
        rc, st = 0, None
        for it in range(repeat):
            if it:
                eng.upload(dB, bimg, bimg.nbytes)
            rc = eng.trsm_raw(n, r, dT, timg.shape[0], dB, bimg.shape[0], side,
                              lower, trans, unit, bool(fp32), check=False)
            if rc:
                break
            st = eng.stats()
            outs.append(fetch(eng, dB, bimg))
        tafter = fetch(eng, dT, timg) if rc == 0 else None
        return rc, outs, st, tafter
    finally:
        for d in bufs:
            eng.free(d)


def run_exact(eng, fp32, form, n, r):
    """One exact case on poisoned images; the record the test asserts on."""
    side, lower, trans, unit = form
    dt = dtype_of(fp32)
    U = UINT[dt]
    t, x, b = exact_problem(side, lower, trans, unit, n, r)
    np_ = r128(n)
    timg = t_image(t, lower, unit, np_ + PAD, dt)
    bimg = b_image(b.astype(dt), side, n, r, (r if side else np_) + PAD, dt)
    rc, outs, st, tafter = solve_images(eng, fp32, form, n, r, timg, bimg)
    rec = {"rc": rc}
    if rc:
        return rec
    got, pad, sent = split_b_image(outs[0], side, n, r)
    want = x.astype(dt)
    # bits, after -0 -> +0 and nothing else (see the head of this file)
    bad = np.argwhere(zero_sign_dropped(got).view(U)
                      != zero_sign_dropped(want).view(U))
    nanbits = _nan(dt).view(U)
    rec.update(
        finite=bool(np.isfinite(got).all()),
        first_bad=[int(v) for v in bad[0]] if len(bad) else None,
        pad_zero=bool((pad == 0).all()),
        sentinels_kept=bool((outs[0].view(U)[sent] == nanbits).all()),
        t_untouched=bool((tafter.view(U) == timg.view(U)).all()),
        flops=st["flops"], launches=st["gemm_launches"])
    return rec


# ---------------------------------------------------------------------------
# the diagonal kernel's arithmetic, restated (test_gpu_diag_bits.py compares
# the device with it bit for bit; test_diag_bits_cpu.py proves it against
# the C++ of marlin_amd/csrc/trsm_plan.h)
def stage_restated(form, t, nv):
    """(L, orig): mx_trsm_stage and mx_trsm_orig in Python. L is the staged
    128 x 128 lower-triangular matrix of the diagonal block t (128 x 128 as
    stored, whatever lies outside the referenced part): the transpose
    resolved, an upper form reversed, 1 on a unit diagonal, the identity at
    an original index >= nv. orig[a] is the original index of canonical a."""
    side, lower, trans, unit = form
    tt = trans ^ side
    rev = 0 if (lower ^ tt) else 1
    orig = (W - 1 - np.arange(W)) if rev else np.arange(W)
    a, b = np.indices((W, W))
    oa, ob = orig[a], orig[b]
    inside = (a >= b) & (oa < nv) & (ob < nv)
    load = inside & ~((a == b) & bool(unit))
    src = t[ob, oa] if tt else t[oa, ob]
    L = np.where(load, src, (a == b).astype(t.dtype)).astype(t.dtype)
    return L, orig


def block_images(fp32, form, n, r=W):
    """(T image, B image) of a one-block case (n <= 128) on rounding data:
    rounding_problem on poisoned images with padded pitches."""
    side, lower, trans, unit = form
    dt = dtype_of(fp32)
    t, b = rounding_problem(fp32, side, lower, trans, n, r)
    return (t_image(t, lower, unit, W + PAD, dt),
            b_image(b, side, n, r, (r if side else W) + PAD, dt))


def block_of_images(form, timg, bimg, r=W):
    """(the 128 x 128 diagonal block as stored, the strip) inside them."""
    strip = bimg[:r, :W] if form[0] else bimg[:W, :r]
    return np.asfortranarray(timg[:W, :W]), np.asfortranarray(strip)


MODELS = ("fused", "unfused", "reciprocal", "reversed")


def substitute_restated(form, t, b, nv, model="fused"):
    """What trsm_diag_kernel leaves in the strip b (128 x r on the left,
    r x 128 on the right) for the diagonal block t, in t's element type.
    Right-looking, b ascending: y_b = mx_trsm_quot(acc_b, L[b][b]), then
    acc_a = mx_trsm_update(acc_a, L[a][b], y_b) = fma(-L[a][b], y_b, acc_a)
    for every a > b at once: an element sees its updates in ascending b,
    the kernel's order. `model` degrades it on purpose, for the tests that
    show such a kernel would be told apart: "unfused" rounds the product
    before the subtraction, "reciprocal" multiplies by 1 / L[b][b],
    "reversed" gives each element its updates in descending b."""
    import _fma
    assert model in MODELS
    side = form[0]
    dt = t.dtype.type
    L, orig = stage_restated(form, np.asarray(t), nv)
    acc = np.array(b.T[orig, :] if side else b[orig, :], dtype=dt, order="C")
    with np.errstate(all="ignore"):
        if model == "reversed":
            for a in range(W):
                for c in range(a - 1, -1, -1):
                    acc[a] = _fma.fma(-L[a, c], acc[c], acc[a])
                acc[a] = acc[a] / L[a, a]
        else:
            for c in range(W):
                if model == "reciprocal":
                    acc[c] = acc[c] * (dt(1) / L[c, c])
                else:
                    acc[c] = acc[c] / L[c, c]
                l, y = L[c + 1:, c][:, None], acc[c][None, :]
                if dt is np.float64:
                    assert _fma.in_range64(l, y, addend=acc[c + 1:]), \
                        "outside the range fma64 is valid in"
                if model == "unfused":
                    acc[c + 1:] = acc[c + 1:] - l * y
                else:
                    acc[c + 1:] = _fma.fma(-l, y, acc[c + 1:])
    out = np.empty_like(acc)
    out[orig, :] = acc
    return np.asfortranarray(out.T if side else out)


def residual_ratio(fp32, form, t, b, x):
    """max over the components of |op(T) X - B| / (2 (n + 2) u |op(T)| |X|),
    in np.longdouble: <= 1 is the backward-error bound of substitution
    (Higham, Accuracy and Stability, Thm 8.5) carried through block updates
    in the conventional order, the factor 2 for evaluating the residual."""
    side, _, trans, _ = form
    ld = np.longdouble
    n = t.shape[0]
    u = ld(2.0) ** (-24 if fp32 else -53)
    op = (t.T if trans else t).astype(ld)
    xl, bl = x.astype(ld), b.astype(ld)
    res = np.abs((xl @ op if side else op @ xl) - bl)
    scale = (np.abs(xl) @ np.abs(op)) if side else (np.abs(op) @ np.abs(xl))
    bound = 2 * (n + 2) * u * scale
    return float(np.max(res / bound))
