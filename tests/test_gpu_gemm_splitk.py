# The split-K GEMM entry (mx_gemm_device_splitk): k cut into slices that
# run as one grouped launch, summed by a second kernel in slice order.
#   1. exact integers (tests/_splitk_cases.EXACT_SHAPES) for both types,
#      both betas and the four op forms: the product, the untouched pad
#      rows / guard column, the reported S and grid;
#   2. the fold spec on rounding data: bit-identity with the numpy left
#      fold of the plain entry's per-slice products;
#   3. slices = 1 is the plain entry's launch, bit for bit;
#   4. refusals touch no buffer;
#   5. empty shapes;
#   6. slices = 0: the auto policy's S for this device, exact result;
#   7. Engine.gemm_dd(split_k=) and computeGramianMatrix(split_k=);
#   8. the workspace across calls of different size on one context;
#   9. both k-loops (two fresh children, gemm_splitk_worker.py, one after
#      the other) give the bits of group 2.
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact
import _splitk_cases as SK
from _exact import Case
from marlin_amd import DenseVecMatrix, Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_splitk_worker.py")
EINVAL = -4

# Once a GPU process of this module has faulted, timed out or died by a
# signal, nothing further is started on the device: every remaining test
# fails immediately with the first failure's reason.
_GPU_POISONED = []


def _require_healthy():
    if _GPU_POISONED:
        pytest.fail("not run: an earlier GPU process of this module "
                    f"failed hard ({_GPU_POISONED[0]})", pytrace=False)


def _rc_ok(rec, what):
    if rec["rc"] == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure")
    assert rec["rc"] == 0, f"{what}: entry returned {rec['rc']}"


@pytest.fixture(scope="module")
def eng():
    _require_healthy()
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def folds(eng):
    """{case id: record} of group 2 in this process, computed once (group 9
    compares the children with it)."""
    out = {}
    for case in SK.FOLD_CASES:
        _require_healthy()
        out[SK.fold_id(*case)] = rec = SK.run_fold(eng, *case)
        if rec["rc"] == -2:
            _GPU_POISONED.append(f"fold {SK.fold_id(*case)}: HIP failure")
            break
    return out


def _fetch(eng, d, like):
    got = np.empty_like(like)
    eng.download(got, d, got.nbytes)
    return got


# ---------------------------------------------------------------------------
# 1. exact integers
@pytest.mark.parametrize("shape", SK.EXACT_SHAPES,
                         ids=[SK.shape_id(s) for s in SK.EXACT_SHAPES])
@pytest.mark.parametrize("fp32,beta,form", SK.COMBOS,
                         ids=[SK.combo_id(*c) for c in SK.COMBOS])
def test_splitk_exact(eng, fp32, beta, form, shape):
    _require_healthy()
    m, n, k, asked, eff = shape
    what = f"{SK.combo_id(fp32, beta, form)} {SK.shape_id(shape)}"
    res = SK.run_exact(eng, fp32, beta, form, m, n, k, asked)
    _rc_ok(res, what)
    assert res["ok"], f"{what}: first mismatch at (row, col) {res['first_bad']}"
    assert not res["sentinel_inside"], f"{what}: sentinel left inside C"
    assert res["pad_ok"], f"{what}: pad rows / guard column overwritten"
    tiles = (m // 128) * (n // 128)
    elem = 4 if fp32 else 8
    assert res["splitk"] == [eff, (eff if beta else eff - 1) * m * n * elem]
    assert res["group"] == [eff, eff * tiles]
    assert res["op"] == list(SK.FORMS[form])
    assert res["launches"] == 1
    assert res["flops"] == 2.0 * m * n * k
    # the grouped launch runs without accumulation: the reduce adds C
    assert res["cfg"]["is_fp32"] == fp32 and res["cfg"]["beta_one"] == 0


# ---------------------------------------------------------------------------
# 2. the fold spec
@pytest.mark.parametrize("fp32,form,s,beta", SK.FOLD_CASES,
                         ids=[SK.fold_id(*c) for c in SK.FOLD_CASES])
def test_splitk_is_left_fold_of_plain_slices(folds, fp32, form, s, beta):
    cid = SK.fold_id(fp32, form, s, beta)
    assert cid in folds, f"{cid}: not run"
    rec = folds[cid]
    _rc_ok(rec, cid)
    assert rec["real"], f"{cid}: not a rounding product near the unsplit one"
    assert rec["equal"], f"{cid}: bits differ from the fold of the slices"
    assert rec["splitk"][0] == s
    assert rec["group"] == [s, 2 * s]


# ---------------------------------------------------------------------------
# 3. slices = 1
@pytest.mark.parametrize("fp32", [0, 1])
@pytest.mark.parametrize("beta", [0, 1])
def test_splitk_one_slice_is_the_plain_entry(eng, fp32, beta):
    _require_healthy()
    dt = _exact.dtype_of(fp32)
    U = _exact.UINT[dt]
    a, b, c0 = SK.fold_inputs(fp32)
    m, n, k = SK.FOLD_M, SK.FOLD_N, SK.FOLD_K
    bufs = []
    try:
        dA, dB = _exact._dev(eng, a, bufs), _exact._dev(eng, b, bufs)
        dP, dS = _exact._dev(eng, c0, bufs), _exact._dev(eng, c0, bufs)
        _rc_ok({"rc": SK._plain(eng, fp32, beta, 0, 0, m, k, n, dA, m, dB, k,
                                dP, m)}, "plain")
        cfg = eng.last_gemm_config()
        # a split call first, so that (1, 0) below is this call's report
        _rc_ok({"rc": eng.gemm_splitk_raw(m, k, n, dA, m, dB, k, dS, m, 2,
                                          fp32, beta, check=False)}, "S = 2")
        assert eng.last_gemm_splitk()[0] == 2
        eng.upload(dS, c0, c0.nbytes)
        _rc_ok({"rc": eng.gemm_splitk_raw(m, k, n, dA, m, dB, k, dS, m, 1,
                                          fp32, beta, check=False)}, "S = 1")
        st = eng.stats()
        assert st["gemm_launches"] == 1 and st["flops"] == 2.0 * m * n * k
        assert eng.last_gemm_splitk() == (1, 0)
        assert eng.last_gemm_config() == cfg
        np.testing.assert_array_equal(_fetch(eng, dS, c0).view(U),
                                      _fetch(eng, dP, c0).view(U))
        # k of one step: any explicit count clamps to the plain launch
        eng.upload(dS, c0, c0.nbytes)
        eng.upload(dP, c0, c0.nbytes)
        assert SK._plain(eng, fp32, beta, 0, 0, m, 16, n, dA, m, dB, k,
                         dP, m) == 0
        assert eng.gemm_splitk_raw(m, 16, n, dA, m, dB, k, dS, m, 4, fp32,
                                   beta, check=False) == 0
        assert eng.last_gemm_splitk() == (1, 0)
        np.testing.assert_array_equal(_fetch(eng, dS, c0).view(U),
                                      _fetch(eng, dP, c0).view(U))
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# 4. refusals
def test_splitk_refusals_touch_nothing(eng):
    _require_healthy()
    U = np.uint64
    c = Case(0, 0, 128, 128, 128)
    a, b, _, _ = _exact.gemm_inputs(c)
    # C: pitch 128 + PAD and a guard column, the NaN sentinel everywhere
    ldc = 128 + _exact.PAD
    cimg = _exact._filled(ldc, 129, _exact._nan(np.float64))
    bufs = []
    try:
        dA, dB = _exact._dev(eng, a, bufs), _exact._dev(eng, b, bufs)
        dC = _exact._dev(eng, cimg, bufs)

        def call(m=128, k=128, n=128, A=dA, lda=128, B=dB, ldb=128, C=dC,
                 ldc=ldc, s=2, ta=0, tb=0):
            return eng.gemm_splitk_raw(m, k, n, A, lda, B, ldb, C, ldc, s,
                                       False, False, ta, tb, check=False)
        refused = {
            "dC == dA": dict(C=dA, ldc=128),
            "dC == dB": dict(C=dB, ldc=128),
            "C two pitch elements past its buffer": dict(ldc=ldc + 2),
            "A one k-step past its buffer": dict(k=144, ldb=144),
            "m not a multiple of 128": dict(m=64),
            "k not a multiple of 16": dict(k=40),
            "ldc not a multiple of 16 bytes": dict(ldc=129),
            "lda below m": dict(lda=126),
            "trans_a = 2": dict(ta=2),
            "trans_b = -1": dict(tb=-1),
        }
        for what, kw in refused.items():
            for s in (2, 0, 1):               # explicit, auto, unsplit
                assert call(s=s, **kw) == EINVAL, f"{what}, slices={s}"
                assert eng.stats()["gemm_launches"] == 0, what
        assert call(s=-1) == EINVAL
        assert eng.stats()["gemm_launches"] == 0
        for d, img in ((dC, cimg), (dA, a), (dB, b)):
            np.testing.assert_array_equal(_fetch(eng, d, img).view(U),
                                          img.view(U))
        # the call they all neighbour passes
        assert call() == 0
        assert eng.last_gemm_splitk() == (2, 128 * 128 * 8)
    finally:
        for d in bufs:
            eng.free(d)


def test_last_gemm_splitk_argument_check(eng):
    _require_healthy()
    import ctypes
    from marlin_amd import engine as E
    s, b = ctypes.c_int(), ctypes.c_int64()
    lib = E.lib()
    assert lib.mx_last_gemm_splitk(None, ctypes.byref(s), ctypes.byref(b)) == -4
    assert lib.mx_last_gemm_splitk(eng._ctx, None, ctypes.byref(b)) == -4
    assert lib.mx_last_gemm_splitk(eng._ctx, ctypes.byref(s), None) == -4


# ---------------------------------------------------------------------------
# 5. empty shapes
@pytest.mark.parametrize("s", [0, 1, 4])
def test_splitk_empty_shapes(eng, s):
    _require_healthy()
    U = np.uint64
    c = Case(0, 0, 128, 128, 128)
    a, b, _, _ = _exact.gemm_inputs(c)
    cimg = _exact._filled(128 + _exact.PAD, 129, _exact._nan(np.float64))
    ldc = cimg.shape[0]
    bufs = []
    try:
        dA, dB = _exact._dev(eng, a, bufs), _exact._dev(eng, b, bufs)
        dC = _exact._dev(eng, cimg, bufs)

        def call(m, k, n, beta):
            return eng.gemm_splitk_raw(m, k, n, dA, 128, dB, 128, dC, ldc, s,
                                       False, beta, check=False)
        for m, n in ((0, 128), (128, 0), (0, 0)):
            for beta in (0, 1):
                assert call(m, 128, n, beta) == 0
                st = eng.stats()
                assert st["gemm_launches"] == 0 and st["gemm_ms"] == 0
                assert eng.last_gemm_splitk() == (1, 0)
        np.testing.assert_array_equal(_fetch(eng, dC, cimg).view(U),
                                      cimg.view(U))
        # k == 0: C unchanged when accumulating, its m x n region cleared
        # (pad rows and guard column kept) otherwise
        assert call(128, 0, 128, 1) == 0
        np.testing.assert_array_equal(_fetch(eng, dC, cimg).view(U),
                                      cimg.view(U))
        assert call(128, 0, 128, 0) == 0
        assert eng.last_gemm_splitk() == (1, 0)
        want = cimg.copy()
        want[:128, :128] = 0
        np.testing.assert_array_equal(_fetch(eng, dC, cimg).view(U),
                                      want.view(U))
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# 6. auto
def test_splitk_auto_policy_on_this_device(eng):
    _require_healthy()
    cus = eng.device_info()[0]
    m, n, k = 128, 128, 4096
    want = SK.auto_slices(0, m, n, k, cus)
    assert want > 1, (cus, SK.min_ksteps())
    res = SK.run_exact(eng, 0, 0, "nn", m, n, k, 0)
    _rc_ok(res, "auto")
    assert res["ok"] and res["pad_ok"] and not res["sentinel_inside"]
    assert res["splitk"] == [want, (want - 1) * m * n * 8]
    assert res["group"] == [want, want]
    # too shallow a k to leave two slices their depth: the plain launch
    kmin = 16 * (2 * SK.min_ksteps() - 1)
    assert SK.auto_slices(0, m, n, kmin, cus) == 1
    res = SK.run_exact(eng, 0, 0, "nn", m, n, kmin, 0)
    _rc_ok(res, "auto, shallow")
    assert res["ok"] and res["splitk"] == [1, 0]


# ---------------------------------------------------------------------------
# 7. layers
def test_gemm_dd_split_k_ragged_gram(eng):
    _require_healthy()
    a, _ = _exact.exact_matrix(1000, 90, 0x6A17, False)
    ref = a.T @ a
    dA = eng.upload_matrix(a)
    try:
        G = eng.gemm_dd(dA, dA, trans_a=True, split_k=3)
        try:
            assert eng.last_gemm_splitk() == (3, 2 * 128 * 128 * 8)
            assert eng.last_gemm_group() == (3, 3)
            assert eng.last_gemm_op() == (1, 0)
            img = np.empty((G.pitch, 128), dtype=np.float64, order="F")
            eng.download(img, G.buf, img.nbytes)
        finally:
            G.free()
        np.testing.assert_array_equal(img[:90, :90], ref)
        assert not img[90:, :].any() and not img[:, 90:].any()
        # the same handle route without the argument is today's call
        G2 = eng.gemm_dd(dA, dA, trans_a=True)
        try:
            assert eng.last_gemm_splitk() == (3, 2 * 128 * 128 * 8)
            np.testing.assert_array_equal(eng.download_matrix(G2), ref)
        finally:
            G2.free()
        G3 = eng.gemm_dd(dA, dA, trans_a=True, split_k="auto")
        try:
            assert eng.last_gemm_splitk()[0] == SK.auto_slices(
                0, 128, 128, 1008, eng.device_info()[0])
            np.testing.assert_array_equal(eng.download_matrix(G3), ref)
        finally:
            G3.free()
    finally:
        dA.free()


def test_compute_gramian_matrix_split_k(eng):
    _require_healthy()
    from oracle import gen_matrix
    a = gen_matrix(500, 90, seed=0x6A18)
    g = DenseVecMatrix(a, engine=eng).computeGramianMatrix(split_k=4)
    assert eng.last_gemm_splitk()[0] == 4
    assert eng.last_gemm_op() == (1, 0)
    ref = a.T @ a
    assert g.shape == (90, 90)
    assert np.max(np.abs(g - ref)) / np.max(np.abs(ref)) < 1e-10


# ---------------------------------------------------------------------------
# 8. workspace
def test_splitk_workspace_across_calls(eng):
    _require_healthy()
    for (m, n, k, s) in ((128, 128, 128, 8), (128, 128, 128, 2),
                         (256, 384, 128, 8)):
        for beta in (0, 1):
            what = f"{m}x{n}x{k} S={s} beta={beta}"
            res = SK.run_exact(eng, 0, beta, "nn", m, n, k, s)
            _rc_ok(res, what)
            assert res["ok"], f"{what}: mismatch at {res['first_bad']}"
            assert res["pad_ok"] and not res["sentinel_inside"], what
            assert res["splitk"] == [s, (s if beta else s - 1) * m * n * 8]
            assert res["group"] == [s, s * (m // 128) * (n // 128)]


# ---------------------------------------------------------------------------
# 9. both k-loops
def _run_worker(loop):
    _require_healthy()
    env = {k: v for k, v in os.environ.items() if k not in SK.KNOBS}
    env.update(SK.LOOPS[loop])
    try:
        r = subprocess.run([sys.executable, WORKER], env=env, timeout=180,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _GPU_POISONED.append(f"{loop}: worker timed out")
        pytest.fail(f"{loop}: worker timed out", pytrace=False)
    if r.returncode < 0 or r.returncode in (134, 139) \
            or "illegal memory access" in r.stderr:
        _GPU_POISONED.append(f"{loop}: worker exit {r.returncode}")
    assert r.returncode == 0, f"{loop}: exit {r.returncode}\n{r.stderr[-2000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.parametrize("loop", list(SK.LOOPS))
def test_splitk_bits_under_each_loop(folds, loop):
    rec = _run_worker(loop)
    assert rec["first"] == [0, 0]        # before the first call of a process
    for case in SK.FOLD_CASES:
        cid = SK.fold_id(*case)
        what = f"{cid}/{loop}"
        assert cid in rec["fold"], f"{what}: not run"
        child = rec["fold"][cid]
        _rc_ok(child, what)
        assert child["loop"] == (1 if loop == "pipe" else 0), what
        assert child["equal"] and child["real"], what
        _rc_ok(folds[cid], cid)
        assert child["digest"] == folds[cid]["digest"], what
