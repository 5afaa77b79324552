# Cases of the grouped GEMM entry (mx_gemm_device_grouped), shared by
# test_gpu_gemm_grouped.py and its child gemm_grouped_worker.py. The exact
# method, inputs and image check are tests/_exact.py's: small integer data
# on which every product and partial sum is representable, so each C is
# compared with assert_array_equal against the exact product.
import numpy as np

import _exact
import _exact_op
from _exact import Case

# (m, n, k): a single tile with only the peeled last k-step, two steps,
# the steady state, a row and a column of blocks, 3 x 2 blocks over 5
# steps, and the ragged second band (nbn = 9) / ragged supertile (nbm = 9)
SHAPES = [(128, 128, 16), (128, 128, 32), (256, 128, 48), (128, 384, 16),
          (384, 256, 80), (128, 1152, 32), (1152, 128, 32)]
BLOCKS = sum((m // 128) * (n // 128) for m, n, _ in SHAPES)
assert BLOCKS == 31
FORMS = dict(nn=(0, 0), **_exact_op.FORMS)
COMBOS = [(fp32, beta, form) for fp32 in (0, 1) for beta in (0, 1)
          for form in FORMS]
LOOPS = {"twobar": {"MARLIN_GEMM_LOOP": "twobar"},
         "pipe": {"MARLIN_GEMM_LOOP": "pipe"}}
KNOBS = ("MARLIN_GEMM_CFG", "MARLIN_GEMM_REMAP", "MARLIN_GEMM_BAND",
         "MARLIN_GEMM_PHASE", "MARLIN_GEMM_LOOP")


def combo_id(fp32, beta, form):
    return f"{'f32' if fp32 else 'f64'}-b{beta}-{form}"


def row(m, k, n, dA, a_off, lda, dB, b_off, ldb, dC, c_off, ldc):
    """One tuple of Engine.gemm_grouped_raw."""
    return (m, k, n, dA, a_off, lda, dB, b_off, ldb, dC, c_off, ldc)


def fail(rc):
    return {"rc": rc, "problems": []}


# ---------------------------------------------------------------------------
# 1. exact, heterogeneous: one call over SHAPES
def run_exact_group(eng, fp32, beta, form):
    """All of SHAPES in one grouped call as C (+)= op(A)·op(B). Pitches
    are rows + PAD, A/B pad rows hold NaN, each C carries its sentinel in
    the pad rows and one guard column."""
    ta, tb = FORMS[form]
    dt = _exact.dtype_of(fp32)
    nan = _exact._nan(dt)
    bufs, rows, imgs = [], [], []
    try:
        for (m, n, k) in SHAPES:
            c = Case(fp32, beta, m, n, k)
            a, b, c0, ref = _exact.gemm_inputs(c)
            sa, sb = _exact_op.stored(a, ta), _exact_op.stored(b, tb)
            lda, ldb = sa.shape[0] + _exact.PAD, sb.shape[0] + _exact.PAD
            cimg, sentinel = _exact_op._c_image(c, c0, dt)
            dA = _exact._dev(eng, _exact._padded(sa, lda, 0, nan), bufs)
            dB = _exact._dev(eng, _exact._padded(sb, ldb, 0, nan), bufs)
            dC = _exact._dev(eng, cimg, bufs)
            rows.append(row(m, k, n, dA, 0, lda, dB, 0, ldb, dC, 0,
                            cimg.shape[0]))
            imgs.append((dC, cimg, ref, sentinel))
        rc = eng.gemm_grouped_raw(rows, fp32, beta, ta, tb, check=False)
        if rc != 0:
            return fail(rc)
        out = {"rc": 0, "problems": [], "group": list(eng.last_gemm_group()),
               "cfg": eng.last_gemm_config(), "loop": eng.last_gemm_loop(),
               "op": list(eng.last_gemm_op())}
        st = eng.stats()
        out["launches"], out["flops"] = st["gemm_launches"], st["flops"]
        for (m, n, k), (dC, cimg, ref, sentinel) in zip(SHAPES, imgs):
            got = np.empty_like(cimg)
            eng.download(got, dC, got.nbytes)
            out["problems"].append(_exact._check_image(
                got, m, n, ref, sentinel.view(_exact.UINT[dt])))
        return out
    finally:
        for d in bufs:
            eng.free(d)


def expected_flops(shapes):
    return float(sum(2 * m * n * k for m, n, k in shapes))


# ---------------------------------------------------------------------------
# 2. bit-identity with the plain entry on ordinary (non-integer) data
def _bits_inputs(fp32):
    """[(tag, ta, tb, m, k, n, ia, ib)] + images: SHAPES as NN, three
    problems sharing one A, and one Gram problem (dA == dB, trans_a)."""
    from oracle import gen_matrix
    dt = _exact.dtype_of(fp32)

    def g(r, c, s):
        return np.asfortranarray(gen_matrix(r, c, seed=s, dtype=dt))
    imgs, probs = [], []
    for i, (m, n, k) in enumerate(SHAPES):
        imgs += [g(m, k, 0xA00 + i), g(k, n, 0xB00 + i)]
        probs.append((m, k, n, len(imgs) - 2, len(imgs) - 1))
    # one A (128 x 16, problem 0's) shared by three problems
    for j in range(2):
        imgs.append(g(16, 128 * (j + 1), 0xC00 + j))
        probs.append((128, 16, 128 * (j + 1), 0, len(imgs) - 1))
    return imgs, probs


def run_bits(eng, fp32, beta):
    """The grouped call against mx_gemm_device_op problem by problem, on
    the same device inputs: {"rc", "equal": [...], "one": bool,
    "gram": bool}. Every C starts as the same gen_matrix image."""
    from marlin_amd import engine as E
    from oracle import gen_matrix
    dt = _exact.dtype_of(fp32)
    U = _exact.UINT[dt]
    imgs, probs = _bits_inputs(fp32)
    bufs = []

    def plain(ta, tb, m, k, n, dA, lda, dB, ldb, dC):
        return E.lib().mx_gemm_device_op(eng._ctx, fp32, beta, ta, tb, m, k,
                                         n, dA, lda, dB, ldb, dC, m)

    def fetch(d, like):
        got = np.empty_like(like)
        eng.download(got, d, got.nbytes)
        return got.view(U)
    try:
        dev = [_exact._dev(eng, x, bufs) for x in imgs]
        c0s = [np.asfortranarray(gen_matrix(m, n, seed=0xD00 + i, dtype=dt))
               for i, (m, k, n, _, _) in enumerate(probs)]
        want = []
        for (m, k, n, ia, ib), c0 in zip(probs, c0s):
            dC = _exact._dev(eng, c0, bufs)
            rc = plain(0, 0, m, k, n, dev[ia], m, dev[ib], k, dC)
            if rc != 0:
                return {"rc": rc}
            want.append(fetch(dC, c0))
        dCs = [_exact._dev(eng, c0, bufs) for c0 in c0s]
        rows = [row(m, k, n, dev[ia], 0, m, dev[ib], 0, k, dC, 0, m)
                for (m, k, n, ia, ib), dC in zip(probs, dCs)]
        rc = eng.gemm_grouped_raw(rows, fp32, beta, check=False)
        if rc != 0:
            return {"rc": rc}
        group = list(eng.last_gemm_group())
        equal = [bool((fetch(dC, c0) == w).all())
                 for dC, c0, w in zip(dCs, c0s, want)]
        # a real product, not equal blanks
        real = all(np.isfinite(w.view(dt)).all() and (w.view(dt) > 0).all()
                   for w in want)
        # a group of one against the plain entry (problem 4: 6 blocks)
        m, k, n, ia, ib = probs[4]
        d1 = _exact._dev(eng, c0s[4], bufs)
        rc = eng.gemm_grouped_raw([row(m, k, n, dev[ia], 0, m, dev[ib], 0, k,
                                       d1, 0, m)], fp32, beta, check=False)
        if rc != 0:
            return {"rc": rc}
        one = bool((fetch(d1, c0s[4]) == want[4]).all())
        one_group = list(eng.last_gemm_group())
        # Gram form: S stored 48 x 384, C = S^T·S with dA == dB, beside a
        # second problem in the same call
        s = np.asfortranarray(gen_matrix(48, 384, seed=0xE00, dtype=dt))
        cg = np.asfortranarray(gen_matrix(384, 384, seed=0xE01, dtype=dt))
        dS = _exact._dev(eng, s, bufs)
        dP, dG, dG2 = (_exact._dev(eng, cg, bufs) for _ in range(3))
        rc = plain(1, 0, 384, 48, 384, dS, 48, dS, 48, dP)
        if rc != 0:
            return {"rc": rc}
        rc = eng.gemm_grouped_raw(
            [row(384, 48, 384, dS, 0, 48, dS, 0, 48, dG, 0, 384),
             row(384, 48, 384, dS, 0, 48, dS, 0, 48, dG2, 0, 384)],
            fp32, beta, trans_a=1, check=False)
        if rc != 0:
            return {"rc": rc}
        wp = fetch(dP, cg)
        gram = bool((fetch(dG, cg) == wp).all() and (fetch(dG2, cg) == wp).all())
        return {"rc": 0, "equal": equal, "real": bool(real), "one": one,
                "gram": gram, "group": group, "one_group": one_group,
                "loop": eng.last_gemm_loop(), "op": list(eng.last_gemm_op())}
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# 3. offsets: A, B and C are rectangles of one 512 x 512 image
IMG, BLK = 512, 128


def offsets_case(fp32):
    """(image, expected image, rows-for-one-buffer builder). Blocks are
    BLK x BLK; C(i, j) += A(i, 0)·B(0, j) for i, j in {2, 3}."""
    dt = _exact.dtype_of(fp32)
    vals, _ = _exact.exact_matrix(IMG, IMG, 0x0FF5E7 + fp32, fp32)
    ld = IMG + _exact.PAD
    img = _exact._padded(vals, ld, 0, _exact._nan(dt))
    want = img.copy()
    v64 = vals.astype(np.float64)
    for i in (2, 3):
        for j in (2, 3):
            r, c = slice(BLK * i, BLK * (i + 1)), slice(BLK * j, BLK * (j + 1))
            want[r, c] = (v64[r, c] + v64[r, :BLK] @ v64[:BLK, c]).astype(dt)

    def rows(d):
        def off(i, j):
            return BLK * j * ld + BLK * i
        return [row(BLK, BLK, BLK, d, off(i, 0), ld, d, off(0, j), ld,
                    d, off(i, j), ld) for i in (2, 3) for j in (2, 3)]
    return img, want, rows


# ---------------------------------------------------------------------------
# 4. many single-tile problems, k cycling 16 / 32 / 48, regions of one C
MANY = 300
MANY_A_COLS, MANY_B_BLOCKS = 48 + 6 * 16, 10


def many_inputs():
    a, _ = _exact.exact_matrix(128, MANY_A_COLS, 0x3A17, False)
    b, _ = _exact.exact_matrix(48, 128 * MANY_B_BLOCKS, 0x3B17, False)
    return a, b


def many_problem(i):
    """(k, first A column, B column block) of problem i."""
    return 16 * (1 + i % 3), 16 * (i % 7), i % MANY_B_BLOCKS


def run_many(eng, dA, dB, a, b, idxs):
    """Problems idxs in one grouped fp64 call, region t of a fresh
    NaN-filled C (pitch 128 + PAD) for the t-th of them. Returns
    (rc, whole image equal to the expected one bit for bit)."""
    dt = np.float64
    nan = _exact._nan(dt)
    lda, ldb, ldc = 128 + _exact.PAD, 48 + _exact.PAD, 128 + _exact.PAD
    cimg = _exact._filled(ldc, 128 * len(idxs) + 1, nan)
    want = cimg.copy()
    rows = []
    dC = eng.alloc(cimg.nbytes)
    try:
        eng.upload(dC, cimg, cimg.nbytes)
        for t, i in enumerate(idxs):
            k, a0, bb = many_problem(i)
            rows.append(row(128, k, 128, dA, a0 * lda, lda,
                            dB, 128 * bb * ldb, ldb, dC, 128 * t * ldc, ldc))
            want[:128, 128 * t:128 * (t + 1)] = (
                a[:, a0:a0 + k] @ b[:k, 128 * bb:128 * (bb + 1)])
        rc = eng.gemm_grouped_raw(rows, False, check=False)
        if rc != 0:
            return rc, False
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
        U = _exact.UINT[dt]
        return 0, bool((got.view(U) == want.view(U)).all())
    finally:
        eng.free(dC)
