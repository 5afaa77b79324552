# Transposed-operand GEMM (mx_gemm_device_op: C (+)= op(A)·op(B) with the
# transposed operand read as stored, staged by the other operand's LDS
# scheme):
#   - exact-integer tables of TN, NT and TT (tests/_exact_op.py) on
#     non-square block grids, pitches larger than the dims, both betas and
#     1/2/3/5 k-tiles, in-process under the default loop and in fresh
#     children under both forced loops and the variant knobs;
#   - raw-bit identity with the plain entry run on host-transposed copies,
#     on random data (same accumulation chain per C element);
#   - the host-side argument guards (rejected before any launch).
# Every comparison is exact equality, never a tolerance.
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact
import _exact_op as XO
import _pipelined_cases as PC
from marlin_amd import Engine
from marlin_amd import engine as E
from oracle import gen_matrix

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_op_worker.py")

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


def _assert_result(res, what):
    if res["rc"] == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure")
    assert res["rc"] == 0, f"{what}: entry returned {res['rc']}"
    assert res["ok"], f"{what}: first mismatch at (row, col) {res['first_bad']}"
    assert not res["sentinel_inside"], f"{what}: sentinel left inside C"
    assert res["pad_ok"], f"{what}: pad rows / trailing column overwritten"


def _assert_default_geometry(res, c, what):
    cfg = res["cfg"]
    assert (cfg["is_fp32"], cfg["beta_one"]) == (c.fp32, c.beta), what
    assert (cfg["bk"], cfg["bm"], cfg["waves"]) == (16, 128, 4), \
        f"{what}: ran {cfg}"


# ---------------------------------------------------------------------------
# 1. exact tables, default knobs, in-process
@pytest.mark.parametrize("form,case", XO.table(),
                         ids=[XO.op_id(f, c) for f, c in XO.table()])
def test_gemm_op_exact(eng, form, case):
    _require_healthy()
    ta, tb = XO.FORMS[form]
    what = XO.op_id(form, case)
    res = XO.run_op_case(eng, case, ta, tb)
    _assert_result(res, what)
    assert res["op"] == [ta, tb], f"{what}: ran op {res['op']}"
    _assert_default_geometry(res, case, what)
    assert res["cfg"]["band"] == min(case.N // 128, 8)
    assert res["loop"] == PC.expected_loop("default", res["cfg"])


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_gemm_op_same_buffer_both_operands(eng, fp32):
    """A^T·A with dA == dB: one stored image in both roles."""
    _require_healthy()
    res = XO.run_alias_case(eng, fp32)
    _assert_result(res, f"alias f{32 if fp32 else 64}")
    assert res["op"] == [1, 0]
    assert (res["cfg"]["bk"], res["cfg"]["bm"], res["cfg"]["waves"]) \
        == (16, 128, 4)


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_gemm_op_plain_form_is_the_plain_entry(eng, fp32):
    """(0, 0) through the new entry: same result record as
    mx_gemm_device_ex on the same case, and op (0, 0) reported."""
    _require_healthy()
    c = _exact.Case(fp32, 1, 384, 2176, 32)
    ref = _exact.run_gemm_case(eng, c)
    _assert_result(ref, _exact.case_id(c))
    res = XO.run_op_case(eng, c, 0, 0)
    _assert_result(res, "nn-" + _exact.case_id(c))
    assert res["op"] == [0, 0]
    assert res["loop"] == PC.expected_loop("default", res["cfg"])
    assert {k: res[k] for k in ref} == ref
    # the op record follows the launch, whichever entry made it
    XO.run_op_case(eng, c, 0, 1)
    assert eng.last_gemm_op() == (0, 1)
    _exact.run_gemm_case(eng, c)
    assert eng.last_gemm_op() == (0, 0)


# ---------------------------------------------------------------------------
# 2. both loops and the variant knobs, one fresh child each
CHILDREN = {
    "twobar": {"MARLIN_GEMM_LOOP": "twobar"},
    "pipe": {"MARLIN_GEMM_LOOP": "pipe"},
    "bk32": {"MARLIN_GEMM_CFG": "bk32"},
    "bm256": {"MARLIN_GEMM_CFG": "bm256"},
    "bands": {"MARLIN_GEMM_REMAP": "bands"},
    "phase1": {"MARLIN_GEMM_PHASE": "1"},
}


@pytest.mark.parametrize("name", list(CHILDREN))
def test_gemm_op_exact_under_knobs(name):
    _require_healthy()
    knobs = CHILDREN[name]
    env = {k: v for k, v in os.environ.items() if k not in PC.KNOBS}
    env.update(knobs)
    try:
        r = subprocess.run([sys.executable, WORKER], env=env, timeout=120,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _GPU_POISONED.append(f"{name}: worker timed out")
        pytest.fail(f"{name}: worker timed out", pytrace=False)
    if r.returncode < 0 or r.returncode in (134, 139) \
            or "illegal memory access" in r.stderr:
        _GPU_POISONED.append(f"{name}: worker exit {r.returncode}")
    assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stderr[-2000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"cases"')]
    assert len(lines) == 1, r.stdout[-2000:]
    got = {c["id"]: c for c in json.loads(lines[0])["cases"]}
    assert set(got) == {XO.op_id(f, c) for f, c in XO.table()}
    loop = name if name in ("twobar", "pipe") else "default"
    for form, c in XO.table():
        ta, tb = XO.FORMS[form]
        what = f"{name} {XO.op_id(form, c)}"
        res = got[XO.op_id(form, c)]
        _assert_result(res, what)
        assert res["op"] == [ta, tb], f"{what}: ran op {res['op']}"
        # bk32 / bm256 must fall back to the default geometry; the band,
        # remap and phase arguments apply as to the plain forms
        assert res["cfg"] == XO.expected_config(knobs, c, ta, tb), \
            f"{what}: ran {res['cfg']}"
        _assert_default_geometry(res, c, what)
        assert res["loop"] == PC.expected_loop(loop, res["cfg"]), \
            f"{what}: ran loop {res['loop']}"


# ---------------------------------------------------------------------------
# 3. bit-identity with NN on a materialised transpose, random data
def _device_c(eng, call, imgs):
    """Upload (A, B, C0) images, run call(dA, dB, dC), download C."""
    bufs = []
    try:
        dA, dB, dC = (_exact._dev(eng, x, bufs) for x in imgs)
        rc = call(dA, dB, dC)
        if rc == -2:
            _GPU_POISONED.append("bits: HIP runtime failure")
        assert rc == 0, f"entry returned {rc}"
        got = np.empty_like(imgs[2])
        eng.download(got, dC, got.nbytes)
        return got
    finally:
        for d in bufs:
            eng.free(d)


@pytest.mark.parametrize("fp32,beta", PC.BITS_CASES,
                         ids=[PC.bits_id(*c) for c in PC.BITS_CASES])
def test_gemm_op_bit_identical_to_nn_on_transposed_copy(eng, fp32, beta):
    _require_healthy()
    m, n, k = PC.BITS_SHAPE
    sa, sb, sc = PC.BITS_SEEDS
    dt = _exact.dtype_of(fp32)
    a, b, c0 = (np.asfortranarray(gen_matrix(r, c, s, dtype=dt))
                for (r, c, s) in ((m, k, sa), (k, n, sb), (m, n, sc)))
    lib = E.lib()
    ref = _device_c(eng, lambda dA, dB, dC: lib.mx_gemm_device_ex(
        eng._ctx, fp32, beta, m, k, n, dA, m, dB, k, dC, m), (a, b, c0))
    assert eng.last_gemm_op() == (0, 0)
    # a real product, not equal blanks (entries are U[0,1))
    assert np.isfinite(ref).all() and (ref > 0).all()
    uref = ref.view(_exact.UINT[dt])
    for form, (ta, tb) in XO.FORMS.items():
        sa_img, sb_img = XO.stored(a, ta), XO.stored(b, tb)
        got = _device_c(eng, lambda dA, dB, dC: lib.mx_gemm_device_op(
            eng._ctx, fp32, beta, ta, tb, m, k, n, dA, sa_img.shape[0], dB,
            sb_img.shape[0], dC, m), (sa_img, sb_img, c0))
        assert eng.last_gemm_op() == (ta, tb)
        assert eng.last_gemm_loop() == (0 if fp32 else 1)   # default loop
        bad = np.argwhere(got.view(uref.dtype) != uref)
        assert len(bad) == 0, (f"{form}: {len(bad)} elements differ from NN "
                               f"on the transposed copy, first at "
                               f"{bad[0].tolist()}")


# ---------------------------------------------------------------------------
# 4. argument guards: every call below is rejected on the host before any
# kernel launch, so the 64-byte buffer is never touched.
def _op_rc(eng, d, fp32, ta, tb, m, k, n, lda, ldb, ldc, beta=0):
    return E.lib().mx_gemm_device_op(eng._ctx, fp32, beta, ta, tb, m, k, n,
                                     d, lda, d, ldb, d, ldc)


def test_gemm_op_argument_guards(eng):
    _require_healthy()
    EINVAL = -4
    lib = E.lib()
    d = eng.alloc(64)
    try:
        for fp32, e16 in ((0, 2), (1, 4)):
            # A^T is k x m: lda must cover k (128 would do for NN at m=128)
            assert _op_rc(eng, d, fp32, 1, 0, 128, 256, 128,
                          128, 256, 128) == EINVAL
            assert _op_rc(eng, d, fp32, 1, 1, 128, 256, 128,
                          128, 128, 128) == EINVAL
            # B^T is n x k: ldb must cover n (32 would do for NN at k=32)
            assert _op_rc(eng, d, fp32, 0, 1, 128, 32, 256,
                          128, 32, 128) == EINVAL
            assert _op_rc(eng, d, fp32, 1, 1, 128, 32, 256,
                          32, 32, 128) == EINVAL
            # ldc is still bounded by m
            assert _op_rc(eng, d, fp32, 1, 1, 256, 32, 128,
                          32, 128, 128) == EINVAL
            # pitches that break 16-byte alignment, each transposed form
            m, k, n = 256, 32, 128
            for ta, tb in XO.FORMS.values():
                lda, ldb = (k if ta else m), (n if tb else k)
                for off in range(1, e16):
                    assert _op_rc(eng, d, fp32, ta, tb, m, k, n, lda + off,
                                  ldb, m) == EINVAL
                    assert _op_rc(eng, d, fp32, ta, tb, m, k, n, lda,
                                  ldb + off, m) == EINVAL
                    assert _op_rc(eng, d, fp32, ta, tb, m, k, n, lda, ldb,
                                  m + off, beta=1) == EINVAL
                # unpadded dims stay rejected
                assert _op_rc(eng, d, fp32, ta, tb, m + 1, k, n,
                              lda + 128, ldb, m + 128) == EINVAL
                assert _op_rc(eng, d, fp32, ta, tb, m, k + 1, n,
                              lda + 16, ldb + 16, m) == EINVAL
                assert _op_rc(eng, d, fp32, ta, tb, m, k, n + 1,
                              lda, ldb + 128, m) == EINVAL
            # trans_x outside {0, 1}
            for bad in (2, -1):
                assert _op_rc(eng, d, fp32, bad, 0, m, k, n, m, k, m) == EINVAL
                assert _op_rc(eng, d, fp32, 0, bad, m, k, n, m, k, m) == EINVAL
                assert _op_rc(eng, d, fp32, bad, 1, m, k, n, k, n, m) == EINVAL
        # null buffers / context
        ctx = eng._ctx
        assert lib.mx_gemm_device_op(ctx, 0, 0, 1, 0, 128, 16, 128, None, 16,
                                     d, 16, d, 128) == EINVAL
        assert lib.mx_gemm_device_op(ctx, 0, 0, 0, 1, 128, 16, 128, d, 128,
                                     None, 128, d, 128) == EINVAL
        assert lib.mx_gemm_device_op(ctx, 0, 0, 1, 1, 128, 16, 128, d, 16,
                                     d, 128, None, 128) == EINVAL
        assert lib.mx_gemm_device_op(None, 0, 0, 1, 1, 128, 16, 128, d, 16,
                                     d, 128, d, 128) == EINVAL
        # mx_last_gemm_op: null out pointers / context
        ta, tb = ctypes.c_int(), ctypes.c_int()
        assert lib.mx_last_gemm_op(ctx, None, ctypes.byref(tb)) == EINVAL
        assert lib.mx_last_gemm_op(ctx, ctypes.byref(ta), None) == EINVAL
        assert lib.mx_last_gemm_op(None, ctypes.byref(ta),
                                   ctypes.byref(tb)) == EINVAL
        # host entry: null buffers, bad trans, empty dims
        x = np.zeros(4)
        xp = x.ctypes.data_as(ctypes.c_void_p)
        assert lib.mx_gemm_op(ctx, 0, 1, 0, 2, 2, 2, None, xp, xp) == EINVAL
        assert lib.mx_gemm_op(ctx, 0, 1, 0, 2, 2, 2, xp, xp, None) == EINVAL
        assert lib.mx_gemm_op(ctx, 0, 2, 0, 2, 2, 2, xp, xp, xp) == EINVAL
        assert lib.mx_gemm_op(ctx, 0, 0, -1, 2, 2, 2, xp, xp, xp) == EINVAL
        assert lib.mx_gemm_op(ctx, 0, 1, 1, 0, 2, 2, xp, xp, xp) == -1
        assert lib.mx_gemm_op(ctx, 1, 0, 1, 2, 2, -3, xp, xp, xp) == -1
    finally:
        eng.free(d)
