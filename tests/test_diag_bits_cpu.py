# The numpy restatements that test_gpu_diag_bits.py compares the diagonal
# kernels with, proven on the CPU: tests/_fma.py against the compiler's
# fma, _getrf_cases.eliminate_restated against mx_getrf_eliminate
# (marlin_amd/csrc/getrf_plan.h) and _trsm_cases.substitute_restated against
# mx_trsm_stage + mx_trsm_substitute (trsm_plan.h), all bit for bit, on
# every class of data the GPU tests use and in both types. The C++ side is
# a stand-alone program (tests/data/diag_bits_check.cpp) built like the plan
# checks: AddressSanitizer + UBSan linked statically, a plain build with a
# warning where the toolchain cannot, and -ffp-contract=off, so that the
# only fused multiply-adds in it are the ones the headers name.
# Each degraded model (a product rounded before the subtraction, a
# multiplication by the reciprocal, the updates of an element in descending
# order) must DIFFER on the same data: a comparison that could not tell them
# apart would pin nothing.
import os
import subprocess
import warnings

import numpy as np
import pytest

import _fma
import _getrf_cases as GC
import _trsm_cases as TC
from _exact import UINT, dtype_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "diag_bits_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")
W = 128


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", *flags, SRC, "-I", INC,
                           "-o", exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("diag_bits")
    exe = str(d / "diag_bits_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        # not silently: the run below then proves less, and says so
        warnings.warn("diag_bits_check built WITHOUT sanitizers, the "
                      "sanitizer link failed: " + r.stderr[-300:])
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    count = [0]

    def run(records):
        """records: a list of lists of arrays (int32 header words and
        element arrays, column-major). Returns the result file's bytes."""
        count[0] += 1
        pin, pout = str(d / f"in{count[0]}"), str(d / f"out{count[0]}")
        with open(pin, "wb") as f:
            for rec in records:
                for part in rec:
                    f.write(np.asarray(part).tobytes(order="F"))
        res = subprocess.run([exe, pin, pout], capture_output=True, text=True,
                             timeout=300)
        assert res.returncode == 0, (res.stdout + res.stderr)[-2000:]
        assert res.stdout.split()[:3] == ["diag_bits", "OK",
                                          str(len(records))]
        with open(pout, "rb") as f:
            return f.read()
    return run


def _i32(*v):
    return np.array(v, dtype=np.int32)


# ---------------------------------------------------------------------------
# 1. the fma helper
def _shift_ulps(z, k):
    I = {np.float32: np.int32, np.float64: np.int64}[z.dtype.type]
    return (z.view(I) + k.astype(I)).view(z.dtype)


def fma_triples(fp32, count=400000):
    """Four classes of `count` / 4 triples each, inside the range the
    helper states for the type: operands of independent magnitude; an addend
    within 60 binades of the product; an addend within 4 ulp of -x * y (the
    cancelling class, where the low half of the product decides every bit of
    the result); and (fp32) products and sums in the subnormal range,
    (fp64) factors with few significant bits, whose products are exact."""
    dt = dtype_of(fp32)
    rng = np.random.RandomState(0xF3A + fp32)
    q = count // 4
    emax = 60 if fp32 else 200

    def val(n, lo, hi):
        m = rng.uniform(1, 2, size=n) * rng.choice([-1.0, 1.0], size=n)
        return np.ldexp(m, rng.randint(lo, hi + 1, size=n))

    with np.errstate(all="ignore"):
        xs, ys, zs = [], [], []
        # independent magnitudes (fp32: overflow and underflow included)
        xs.append(val(q, -emax, emax)); ys.append(val(q, -emax, emax))
        zs.append(val(q, -2 * emax, 2 * emax) if not fp32
                  else val(q, -149, 127))
        # the addend near the product's magnitude
        x, y = val(q, -emax // 2, emax // 2), val(q, -emax // 2, emax // 2)
        x, y = x.astype(dt), y.astype(dt)
        e = np.frexp(x.astype(np.float64) * y.astype(np.float64))[1]
        z = np.ldexp(rng.uniform(1, 2, size=q) * rng.choice([-1.0, 1.0], q),
                     e + rng.randint(-60, 61, size=q))
        xs.append(x); ys.append(y); zs.append(z)
        # cancelling: z = -fl(x y) moved by -4 .. 4 ulp
        x, y = val(q, -20, 20).astype(dt), val(q, -20, 20).astype(dt)
        z = _shift_ulps((-(x * y)).astype(dt), rng.randint(-4, 5, size=q))
        xs.append(x); ys.append(y); zs.append(z)
        if fp32:
            # subnormal results: |x y| and |z| around 2^-140
            x, y = val(q, -80, -60), val(q, -80, -60)
            z = val(q, -149, -130) * rng.choice([0.0, 1.0], size=q)
        else:
            x = rng.randint(-2 ** 20, 2 ** 20, size=q).astype(np.float64)
            y = rng.randint(-2 ** 20, 2 ** 20, size=q).astype(np.float64)
            z = val(q, 0, 60) * rng.choice([0.0, 1.0], size=q)
        xs.append(x); ys.append(y); zs.append(z)
        x, y, z = (np.concatenate([np.asarray(v, dtype=np.float64) for v in g])
                   .astype(dt) for g in (xs, ys, zs))
    return x, y, z


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_fma_helper_equals_the_compilers_fma(program, fp32):
    dt = dtype_of(fp32)
    U = UINT[dt]
    x, y, z = fma_triples(fp32)
    assert len(x) >= 400000
    if not fp32:
        assert _fma.in_range64(x, y, addend=z)
    raw = program([[_i32(0, fp32, len(x)), x, y, z]])
    want = np.frombuffer(raw, dtype=dt)
    got = _fma.fma(x, y, z)
    assert got.dtype == dt
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all()
    bad = np.nonzero(~nan & (got.view(U) != want.view(U)))[0]
    assert len(bad) == 0, (f"{len(bad)} mismatches, first at {bad[0]}: "
                           f"fma({x[bad[0]]!r}, {y[bad[0]]!r}, {z[bad[0]]!r})")
    # the triples do exercise the single rounding: a multiply followed by
    # an add gives other bits on a large part of them
    with np.errstate(all="ignore"):
        plain = (x * y + z).astype(dt)
    differ = np.mean(~nan & (plain.view(U) != want.view(U)))
    print(f"fma {'f32' if fp32 else 'f64'}: 0 of {len(x)} mismatches; a plain "
          f"multiply-add differs on {100 * differ:.1f} %")
    assert differ > 0.2
    # the cancelling class alone
    q = len(x) // 4
    c = slice(2 * q, 3 * q)
    assert np.mean(plain[c].view(U) != want[c].view(U)) > 0.5


# ---------------------------------------------------------------------------
# 2. the elimination
def getrf_classes(fp32):
    """(name, A) of every class of block test_gpu_diag_bits.py factors."""
    out = [(f"normal n={n}", GC.normal_problem(fp32, n))
           for n in (1, 2, 63, 64, 65, 127, 128)]
    if fp32:
        out.append(("subnormal", GC.normal_problem(1, 128, -130)))
    out.append(("nan", GC.nan_problem(fp32)[0]))
    out.append(("inf", GC.inf_problem(fp32)[0]))
    for n in (129, 300):
        out.append((f"leading block of n={n}",
                    GC.normal_problem(fp32, n)[:W, :W]))
    return out


def _block(a, dt):
    blk = np.zeros((W, W), dtype=dt, order="F")
    blk[:a.shape[0], :a.shape[1]] = a
    return blk


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_eliminate_restated_equals_the_header(program, fp32):
    dt = dtype_of(fp32)
    classes = getrf_classes(fp32)
    blocks = [_block(a, dt) for _, a in classes]
    raw = program([[_i32(1, fp32, a.shape[0]), blk]
                   for (_, a), blk in zip(classes, blocks)])
    rec = W * W * dt().itemsize + 4 * W + 4
    assert len(raw) == rec * len(classes)
    for i, ((name, a), blk) in enumerate(zip(classes, blocks)):
        part = raw[i * rec:(i + 1) * rec]
        want = np.frombuffer(part, dtype=dt, count=W * W).reshape(
            (W, W), order="F")
        perm = np.frombuffer(part, dtype=np.int32, count=W + 1,
                             offset=W * W * dt().itemsize)
        got, gperm, gfz = GC.eliminate_restated(blk, a.shape[0])
        bad = GC.same_bits(got, want)
        assert len(bad) == 0, f"{name}: {len(bad)} elements differ"
        np.testing.assert_array_equal(gperm, perm[:W], err_msg=name)
        assert gfz == perm[W] == 0, name
        if a.shape[0] > 2:
            assert (gperm != np.arange(W)).any(), f"{name}: nothing pivoted"
    # the subnormal class is what it says
    if fp32:
        a = GC.normal_problem(1, 128, -130)
        tiny = np.finfo(np.float32).tiny
        assert (np.abs(a) < tiny).mean() > 0.9 and (a != 0).mean() > 0.9


@pytest.mark.parametrize("model", ["unfused", "reciprocal"])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_eliminate_degraded_models_differ(fp32, model):
    # (the elimination has no "reversed" model: an update of step j needs
    # the results of step j - 1)
    a = GC.normal_problem(fp32, 128)
    want, perm, _ = GC.eliminate_restated(a, 128)
    got, _, _ = GC.eliminate_restated(a, 128, model=model)
    differ = len(GC.same_bits(got, want))
    print(f"getrf {model}: {differ} of {W * W} elements differ")
    assert differ > W * W // 4


def test_eliminate_subnormal_class_tells_a_flush_apart():
    # Among subnormals every value is a multiple of 2^-149, the rounded
    # product's error rarely survives the subtraction and the unfused model
    # differs in few elements. What this class is for is a kernel that
    # flushes subnormals to zero: every result would be a zero.
    a = GC.normal_problem(1, 128, -130)
    want, _, _ = GC.eliminate_restated(a, 128)
    tiny = np.finfo(np.float32).tiny
    u = np.triu(want)
    assert ((u != 0) & (np.abs(u) < tiny)).sum() > 128 * 129 // 2 * 0.9
    assert (np.abs(u) < 2.0 ** -120).all()
    l = np.tril(want, -1)
    assert (np.abs(l) <= 1).all() and (np.abs(l) > 2.0 ** -20).mean() > 0.45
    for model in ("unfused", "reciprocal"):
        got, _, _ = GC.eliminate_restated(a, 128, model=model)
        assert len(GC.same_bits(got, want)) > 0, model


def test_eliminate_sinks_a_nan_and_breaks_an_inf_tie_downward():
    for fp32 in (0, 1):
        a, r = GC.nan_problem(fp32)
        got, perm, fz = GC.eliminate_restated(a, 128)
        assert perm[127] == r and fz == 0
        assert np.isfinite(got[:127, :]).all() and np.isnan(got[127, :]).all()
        a, r1, r2 = GC.inf_problem(fp32)
        got, perm, fz = GC.eliminate_restated(a, 128)
        assert perm[0] == r1 and perm[127] == r2 and fz == 0
        assert np.isinf(got[0, 0]) and np.isfinite(got[:127, 1:]).all()
        assert not got[1:127, 0].any() and np.isnan(got[127, :]).all()


# ---------------------------------------------------------------------------
# 3. the substitution
TRSM_ORDERS = (1, 77, 128)


def trsm_block_case(fp32, form, n, r=128):
    """(T block 128 x 128, strip) of the one-block case of
    test_gpu_diag_bits.py: rounding data on poisoned images."""
    timg, bimg = TC.block_images(fp32, form, n, r)
    return TC.block_of_images(form, timg, bimg, r)


def _trsm_record(fp32, form, n, tblk, strip):
    side, lower, trans, unit = form
    tt = trans ^ side
    rev = 0 if (lower ^ tt) else 1
    r = strip.shape[0] if side else strip.shape[1]
    return [_i32(2, fp32, side, tt, rev, unit, n, r), tblk, strip]


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_substitute_restated_equals_the_header(program, fp32):
    dt = dtype_of(fp32)
    cases = [(form, n) + trsm_block_case(fp32, form, n)
             for form in TC.FORMS for n in TRSM_ORDERS]
    # the two strip solves of a blocked LU step, on the packed factors of a
    # block with nothing dominant: L21 = A21 U11^-1 and U12 = L11^-1 A12
    lu, _, _ = GC.eliminate_restated(GC.normal_problem(fp32, 128), 128)
    rng = np.random.RandomState(77 + fp32)
    cases.append(((1, 0, 0, 0), 128, lu,
                  np.asfortranarray(rng.standard_normal((256, W)).astype(dt))))
    cases.append(((0, 1, 0, 1), 128, lu,
                  np.asfortranarray(rng.standard_normal((W, 256)).astype(dt))))
    raw = program([_trsm_record(fp32, form, n, t, s)
                   for form, n, t, s in cases])
    off = 0
    for form, n, t, s in cases:
        want = np.frombuffer(raw, dtype=dt, count=s.size,
                             offset=off).reshape(s.shape, order="F")
        off += s.nbytes
        got = TC.substitute_restated(form, t, s, n)
        what = f"{TC.form_id(form)} n={n}"
        assert np.isfinite(want).all(), f"{what}: poison was read"
        bad = GC.same_bits(got, want)
        assert len(bad) == 0, f"{what}: {len(bad)} elements differ"
    assert off == len(raw)


@pytest.mark.parametrize("model", ["unfused", "reciprocal", "reversed"])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_substitute_degraded_models_differ(fp32, model):
    for form in ((0, 1, 0, 0), (1, 0, 1, 0)):
        for n in (77, 128):
            t, s = trsm_block_case(fp32, form, n)
            want = TC.substitute_restated(form, t, s, n)
            got = TC.substitute_restated(form, t, s, n, model=model)
            differ = len(GC.same_bits(got, want))
            print(f"trsm {TC.form_id(form)} n={n} {model}: {differ} of "
                  f"{n * 128} elements differ")
            assert differ > n * 128 // 4
