# The arithmetic of every entry that reaches gemm_mfma_kernel or the gemv
# kernels, checked componentwise against a high-precision reference of the
# same rounded inputs (tests/_rounding_cases.py states the quantity, the hard
# bound H and the statistics S1 and S2, and derives them; the CPU-only
# test_rounding_cases.py shows that they reject reduced-precision operands,
# a round-toward-zero accumulate and flushed subnormals).
#
# H is a property of IEEE round-to-nearest arithmetic in the element type in
# any summation order, fused or not; no threshold here is taken from a
# measurement (those are in profiles/gemm_rounding.md). Every case prints its
# figures ahead of its assertions.
#
# Images and conventions are tests/_exact.py's: pitches larger than the dims,
# NaN in the pads, C prefilled with a sentinel plus a guard column. Every
# case is 128 x 128 unless stated and none is larger than 256 x 256 x 1056.
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _rounding_cases as RC
from _exact import PAD, _dev, _nan, _padded, dtype_of
from _rounding_cases import KS, M, N
from marlin_amd import Engine
from marlin_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_rounding_worker.py")
TYPES = [0, 1]
_TID = ["f64", "f32"]

# Once a GPU process of this module has faulted, timed out or died by a
# signal, nothing further is started on the device: every remaining test
# fails immediately with the first failure's reason.
_GPU_POISONED = []


def _require_healthy():
    if _GPU_POISONED:
        pytest.fail("not run: an earlier GPU process of this module "
                    f"failed hard ({_GPU_POISONED[0]})", pytrace=False)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _ran(res, what, pads=True):
    if res["rc"] == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure")
    assert res["rc"] == 0, f"{what}: entry returned {res['rc']}"
    if pads:
        assert not res["sentinel_inside"], f"{what}: sentinel left inside C"
        assert res["pad_ok"], f"{what}: pad rows / guard column overwritten"


def _hold(entry, fp32, k, cls, got, r, s, terms, which=None, note=""):
    """Print the figures of one result, then assert the criteria `which`
    (default: those of the class)."""
    mes = RC.measure(got, r, s, fp32, terms)
    print(RC.report_line(entry, fp32, k, cls, mes, note))
    bad = RC.failures(mes, RC.criteria(cls) if which is None else which)
    assert not bad, f"{entry} {_TID[fp32]} k={k} {cls} {note}: {bad}"


# ---------------------------------------------------------------------------
# E1: the plain device entry
@pytest.mark.parametrize("cls", ["pos", "mix", "wide"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("beta", [0, 1], ids=["b0", "b1"])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_device_entry(eng, fp32, beta, k, cls):
    _require_healthy()
    a, b, r, s = RC.product(cls, fp32, M, k, N)
    c0 = RC.operand(cls, "c", fp32, M, N) if beta else None
    if beta:
        r, s = RC.with_addend(r, s, c0, fp32)
    res = RC.run_op(eng, fp32, "nn", a, b, c0)
    _ran(res, f"device {cls} k={k}")
    assert res["cfg"]["beta_one"] == beta and res["op"] == [0, 0]
    _hold("device", fp32, k, cls, res["got"], r, s, k + beta,
          note=f"beta={beta}")


@pytest.mark.parametrize("cls", ["sub_out", "sub_in"])
@pytest.mark.parametrize("k", [16, 64])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_device_entry_subnormals(eng, fp32, k, cls):
    # gradual underflow: subnormal products and results (sub_out), and
    # subnormal inputs (sub_in), are honoured, not flushed
    _require_healthy()
    a, b, r, s = RC.product(cls, fp32, M, k, N)
    res = RC.run_op(eng, fp32, "nn", a, b)
    _ran(res, f"device {cls} k={k}")
    _hold("device", fp32, k, cls, res["got"], r, s, k)


# ---------------------------------------------------------------------------
# E2: the transposed-operand forms
@pytest.mark.parametrize("cls", ["pos", "mix"])
@pytest.mark.parametrize("form", ["tn", "nt", "tt"])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_op_forms(eng, fp32, form, cls):
    _require_healthy()
    k = 64
    a, b, r, s = RC.product(cls, fp32, M, k, N)
    res = RC.run_op(eng, fp32, form, a, b)
    _ran(res, f"op {form} {cls}")
    assert res["op"] == list(RC.FORMS[form])
    _hold(f"op_{form}", fp32, k, cls, res["got"], r, s, k)


# ---------------------------------------------------------------------------
# E3: the latched variants, one fresh child process each
@pytest.mark.parametrize("variant", list(RC.VARIANTS))
def test_latched_variants(variant, tmp_path):
    _require_healthy()
    env = {k: v for k, v in os.environ.items() if k not in RC.KNOBS}
    env.update(RC.VARIANTS[variant])
    try:
        p = subprocess.run([sys.executable, WORKER, variant, str(tmp_path)],
                           env=env, timeout=120, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        _GPU_POISONED.append(f"{variant}: worker timed out")
        pytest.fail(f"{variant}: worker timed out", pytrace=False)
    if p.returncode < 0 or p.returncode in (134, 139) \
            or "illegal memory access" in p.stderr:
        _GPU_POISONED.append(f"{variant}: worker exit {p.returncode}")
    assert p.returncode == 0, \
        f"{variant}: exit {p.returncode}\n{p.stderr[-2000:]}"
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"cases"')]
    assert len(lines) == 1, p.stdout[-2000:]
    got = {c["id"]: c for c in json.loads(lines[0])["cases"]}
    cases = RC.variant_cases(variant)
    assert set(got) == {RC.variant_case_id(c) for c in cases}
    problems = []
    for case in cases:
        fp32, beta, cls, m, n, k = case
        cid = RC.variant_case_id(case)
        res = got[cid]
        _ran(res, f"{variant} {cid}")
        # the variant under test really ran
        bk, bm, loop = RC.variant_expected(variant, fp32)
        cfg = res["cfg"]
        assert (cfg["is_fp32"], cfg["beta_one"], cfg["bk"], cfg["bm"]) == \
            (fp32, beta, bk, bm), f"{variant} {cid}: ran {cfg}"
        assert res["loop"] == loop, f"{variant} {cid}: loop {res['loop']}"
        c = np.load(os.path.join(tmp_path, cid + ".npy"))
        r, s, terms = RC.case_reference(case)
        mes = RC.measure(np.asfortranarray(c), r, s, fp32, terms)
        print(RC.report_line(variant, fp32, k, cls, mes, f"beta={beta}"))
        problems += [f"{cid}: {f}" for f in
                     RC.failures(mes, RC.criteria(cls))]
    assert not problems, f"{variant}: {problems}"


# ---------------------------------------------------------------------------
# E4: the fused transpose(+add) epilogue
@pytest.mark.parametrize("cls", ["pos", "mix"])
@pytest.mark.parametrize("with_add", [False, True], ids=["noadd", "add"])
@pytest.mark.parametrize("k", [16, 272])
def test_fused_epilogue(eng, k, with_add, cls):
    _require_healthy()
    a, b, r, s = RC.product(cls, 1, M, k, N)
    r, s = r.T, s.T
    add = RC.operand("mix", "c", 1, N, M) if with_add else None
    if with_add:
        r, s = RC.with_addend(r, s, add, 1)
    res = RC.run_epilogue(eng, a, b, add)
    _ran(res, f"epilogue {cls} k={k} add={with_add}")
    which = ("H", "S1", "S2") if cls == "pos" and not with_add else ("H",)
    _hold("epilogue", 1, k, cls, res["got"], r, s, k + int(with_add), which,
          note="add" if with_add else "noadd")


# ---------------------------------------------------------------------------
# E5: grouped and split-K
GROUP_KS = (16, 64, 272)


@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_grouped(eng, fp32):
    _require_healthy()
    prods = [RC.product("mix", fp32, M, k, N) for k in GROUP_KS]
    out = RC.run_grouped(eng, fp32, [(p[0], p[1]) for p in prods])
    _ran(out, "grouped", pads=False)
    assert out["group"][0] == len(GROUP_KS)
    problems = []
    for k, (_, _, r, s), res in zip(GROUP_KS, prods, out["problems"]):
        _ran(res, f"grouped k={k}")
        mes = RC.measure(res["got"], r, s, fp32, k)
        print(RC.report_line("grouped", fp32, k, "mix", mes))
        problems += [f"k={k}: {f}" for f in RC.failures(mes, ("H",))]
    assert not problems, problems


@pytest.mark.parametrize("beta", [0, 1], ids=["b0", "b1"])
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_splitk(eng, fp32, beta):
    # S slices change the order: each slice is a chain of its own and the
    # fold adds S - 1 (S when accumulating) roundings: terms = k + S
    _require_healthy()
    k, S = 1040, 4
    a, b, r, s = RC.product("mix", fp32, M, k, N)
    c0 = RC.operand("mix", "c", fp32, M, N) if beta else None
    if beta:
        r, s = RC.with_addend(r, s, c0, fp32)
    res = RC.run_op(eng, fp32, "nn", a, b, c0, slices=S)
    _ran(res, f"splitk beta={beta}")
    assert res["splitk"][0] == S
    _hold("splitk", fp32, k, "mix", res["got"], r, s, k + S, ("H",),
          note=f"S={S} beta={beta}")


# ---------------------------------------------------------------------------
# E6: the SUMMA panel loop; the accumulate chain continues across panels,
# so terms = k
@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_summa_panel_loop(eng, fp32):
    _require_healthy()
    m, k, n, kb = 200, 100, 200, 32
    a, b, r, s = RC.product("mix", fp32, m, k, n)
    res = RC.run_summa_position(eng, fp32, 2, 2, 1, 1, a, b, kb)
    _ran(res, "summa (1, 1) of 2 x 2")
    assert res["panels"] >= 3 and res["launches"] == res["panels"]
    assert res["pad_rows_zero"] and res["pad_cols_zero"]
    (r0, r1), (c0, c1) = res["rows"], res["cols"]
    assert (r0, c0) != (0, 0) and res["got"].shape == (r1 - r0, c1 - c0)
    _hold("summa", fp32, k, "mix", res["got"], r[r0:r1, c0:c1],
          s[r0:r1, c0:c1], k, ("H",), note=f"panels={res['panels']}")


# ---------------------------------------------------------------------------
# E7: the host entries on a ragged shape (the staging pads with zeros,
# which add exact zeros to every chain)
HM, HK, HN = 129, 37, 127


def _host(eng, name, fp32, args, shape):
    dt = dtype_of(fp32)
    got = np.full(shape, np.nan, dtype=dt, order="F")
    rc = getattr(E.lib(), name)(eng._ctx, *args, E._fbuf(got, dt))
    if rc == -2:
        _GPU_POISONED.append(f"{name}: HIP runtime failure")
    assert rc == 0, f"{name} returned {rc}"
    return got


@pytest.mark.parametrize("name,fp32", [("mx_dgemm", 0), ("mx_sgemm", 1)])
def test_host_plain_entries(eng, name, fp32):
    _require_healthy()
    dt = dtype_of(fp32)
    a, b, r, s = RC.product("mix", fp32, HM, HK, HN)
    got = _host(eng, name, fp32,
                (HM, HK, HN, E._fbuf(a, dt), E._fbuf(b, dt)), (HM, HN))
    _hold(name, fp32, HK, "mix", got, r, s, HK, ("H",))


def test_host_gemm_op_tn(eng):
    _require_healthy()
    a, b, r, s = RC.product("mix", 0, HM, HK, HN)
    at = np.asfortranarray(a.T)                      # stored k x m
    got = np.full((HM, HN), np.nan, order="F")
    rc = E.lib().mx_gemm_op(eng._ctx, 0, 1, 0, HM, HK, HN,
                            at.ctypes.data_as(ctypes.c_void_p),
                            b.ctypes.data_as(ctypes.c_void_p),
                            got.ctypes.data_as(ctypes.c_void_p))
    if rc == -2:
        _GPU_POISONED.append("mx_gemm_op: HIP runtime failure")
    assert rc == 0
    _hold("mx_gemm_op_tn", 0, HK, "mix", got, r, s, HK, ("H",))


def test_host_tile_acc_chain(eng):
    # C = A0 B0; C += A1 B1; C += A2 B2: one chain of 3 k summands
    _require_healthy()
    prods = [RC.product("mix", 0, HM, HK, HN, tag) for tag in range(3)]
    c = np.full((HM, HN), np.nan, order="F")
    for i, (a, b, _, _) in enumerate(prods):
        rc = E.lib().mx_tile_dgemm_acc(
            eng._ctx, HM, HK, HN, E._fbuf(a, np.float64),
            E._fbuf(b, np.float64), E._fbuf(c, np.float64), int(i > 0))
        if rc == -2:
            _GPU_POISONED.append("mx_tile_dgemm_acc: HIP runtime failure")
        assert rc == 0
    r = prods[0][2] + prods[1][2] + prods[2][2]
    s = prods[0][3] + prods[1][3] + prods[2][3]
    _hold("mx_tile_dgemm_acc", 0, 3 * HK, "mix", c, r, s, 3 * HK, ("H",),
          note="chain=3")


def test_host_fused_epilogue_with_add(eng):
    _require_healthy()
    f32 = np.float32
    a, b, r, s = RC.product("mix", 1, HM, HK, HN)
    add = RC.operand("mix", "c", 1, HN, HM)
    r, s = RC.with_addend(r.T, s.T, add, 1)
    got = np.full((HN, HM), np.nan, dtype=f32, order="F")
    rc = E.lib().mx_sgemm_epilogue(eng._ctx, HM, HK, HN, E._fbuf(a, f32),
                                   E._fbuf(b, f32), E._fbuf(got, f32), 1,
                                   E._fbuf(add, f32))
    if rc == -2:
        _GPU_POISONED.append("mx_sgemm_epilogue: HIP runtime failure")
    assert rc == 0
    _hold("mx_sgemm_epilogue", 1, HK, "mix", got, r, s, HK + 1, ("H",),
          note="add")


# ---------------------------------------------------------------------------
# E8: gemv (fp64 partial sums per column chunk, reduced in chunk order)
GV_M, GV_N, GV_LDA = 300, 517, 304


@pytest.mark.parametrize("cls", ["mix", "wide"])
@pytest.mark.parametrize("entry", ["mx_dgemv", "mx_dgemv_device"])
def test_gemv(eng, entry, cls):
    _require_healthy()
    a, x, r, s = RC.product(cls, 0, GV_M, GV_N, 1)
    xv = np.ascontiguousarray(x[:, 0])
    if entry == "mx_dgemv":
        y = eng.dgemv(a, xv)
    else:
        bufs = []
        try:
            dA = _dev(eng, _padded(a, GV_LDA, 0, _nan(np.float64)), bufs)
            y = eng.dgemv_device_raw(GV_M, GV_N, dA, GV_LDA, xv)
        finally:
            for d in bufs:
                eng.free(d)
    _hold(entry, 0, GV_N, cls, np.asfortranarray(y.reshape(GV_M, 1)), r, s,
          GV_N, ("H",))


# ---------------------------------------------------------------------------
# E9: special values propagate as IEEE arithmetic says
def _special_inputs(fp32, k):
    """mix operands with +inf, -inf and NaN in distinct rows of A, and one
    +inf in B whose column of partners in A holds an exact 0."""
    a, b, _, _ = RC.product("mix", fp32, M, k, N)
    a, b = np.array(a, order="F"), np.array(b, order="F")
    a[5, 3], a[40, 17], a[77, 60] = np.inf, -np.inf, np.nan
    b[9, 21] = np.inf            # pairs with column 9 of A
    a[100, 9] = 0.0              # 0 * inf = NaN at (100, 21)
    return a, b


@pytest.mark.parametrize("fp32", TYPES, ids=_TID)
def test_special_values(eng, fp32):
    _require_healthy()
    k = 64
    a, b = _special_inputs(fp32, k)
    # the float64 reference of the pattern: plain IEEE sums of products in
    # ascending k (a sum holding +inf and -inf, or a NaN, is NaN in any
    # order; nothing finite overflows here)
    want = np.zeros((M, N))
    with np.errstate(invalid="ignore"):
        for l in range(k):
            want += a[:, l:l + 1].astype(np.float64) * b[l:l + 1, :]
    assert np.isnan(want[100, 21]) and np.isnan(want[77]).all()
    assert np.isinf(want[5]).sum() >= N - 1 and np.isinf(want[:, 21]).any()
    res = RC.run_op(eng, fp32, "nn", a, b)
    _ran(res, "special values")
    got = res["got"]
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf),
                    ("-inf", np.isneginf)):
        diff = np.argwhere(f(got) != f(want))
        assert len(diff) == 0, (f"{name} pattern differs at "
                                f"{diff[:4].tolist()} ({len(diff)} elements)")
    # the finite entries have finite operands all along k: hold them to H
    # against the reference of the operands with the specials removed
    fin = np.isfinite(want)
    rt = RC.ref_type(fp32)
    az = np.where(np.isfinite(a), a, 0).astype(rt)
    bz = np.where(np.isfinite(b), b, 0).astype(rt)
    r, s = az @ bz, np.abs(az) @ np.abs(bz)
    safe = np.where(fin, got, r.astype(got.dtype))
    _hold("special", fp32, k, "mix", np.asfortranarray(safe), r, s, k,
          ("H",), note=f"finite={int(fin.sum())}")
