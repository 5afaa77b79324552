# Exact-arithmetic tests of every gemm_mfma_kernel instantiation, the
# supertiled/plain band remaps, pitches larger than the dims, the fused
# transpose(+add) epilogue, and the host-side argument guards.
#
# Inputs are small signed integers (tests/_exact.py derives the bounds)
# so the exact product is representable and a correct kernel, in any
# accumulation order, returns it bit for bit: every comparison here is
# exact equality, never a tolerance.
import ctypes
import json
import os
import subprocess
import sys

import pytest

import _exact
from marlin_amd import Engine
from marlin_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_cfg_worker.py")

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
        _GPU_POISONED.append(f"{what}: HIP runtime failure in-process")
    assert res["rc"] == 0, f"{what}: entry returned {res['rc']}"
    assert res["ok"], f"{what}: first mismatch at (row, col) {res['first_bad']}"
    assert not res["sentinel_inside"], f"{what}: sentinel left inside C"
    assert res["pad_ok"], f"{what}: pad rows / trailing column overwritten"


# ---------------------------------------------------------------------------
# default config, in-process
@pytest.mark.parametrize("case", _exact.default_cases(), ids=_exact.case_id)
def test_gemm_exact_default_config(eng, case):
    _require_healthy()
    res = _exact.run_gemm_case(eng, case)
    _assert_result(res, _exact.case_id(case))
    cfg = res["cfg"]
    assert (cfg["is_fp32"], cfg["beta_one"]) == (case.fp32, case.beta)
    assert (cfg["bk"], cfg["bm"], cfg["waves"]) == (16, 128, 4)
    assert cfg["band"] == min(case.N // 128, 8) > 0
    assert cfg["phase_mask"] == 0


@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
@pytest.mark.parametrize("K", _exact.EPI_KS)
@pytest.mark.parametrize("grid", _exact.EPI_GRIDS,
                         ids=lambda g: f"{g[0]}x{g[1]}")
def test_sgemm_epilogue_exact(eng, grid, K, with_add):
    _require_healthy()
    M, N = 128 * grid[0], 128 * grid[1]
    res = _exact.run_epilogue_case(eng, M, N, K, with_add)
    _assert_result(res, f"epilogue {M}x{N}x{K} add={with_add}")


# ---------------------------------------------------------------------------
# alternate configs, one fresh child process each
CONFIGS = [
    {"MARLIN_GEMM_CFG": "bk32"},
    {"MARLIN_GEMM_CFG": "bm256"},
    {"MARLIN_GEMM_REMAP": "bands"},
    {"MARLIN_GEMM_BAND": "4"},
    {"MARLIN_GEMM_BAND": "16"},
    {"MARLIN_GEMM_BAND": "3"},
    {"MARLIN_GEMM_PHASE": "1"},
    {"MARLIN_GEMM_PHASE": "8"},
    {"MARLIN_GEMM_CFG": "bk32", "MARLIN_GEMM_PHASE": "1"},
]
_KNOBS = ("MARLIN_GEMM_CFG", "MARLIN_GEMM_REMAP", "MARLIN_GEMM_BAND",
          "MARLIN_GEMM_PHASE")


def _cfg_id(cfg):
    return "+".join(f"{k[len('MARLIN_GEMM_'):]}={v}" for k, v in cfg.items())


@pytest.mark.parametrize("knobs", CONFIGS, ids=_cfg_id)
def test_gemm_exact_alternate_config(knobs):
    _require_healthy()
    env = {k: v for k, v in os.environ.items() if k not in _KNOBS}
    env.update(knobs)
    what = _cfg_id(knobs)
    try:
        r = subprocess.run([sys.executable, WORKER], env=env, timeout=120,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _GPU_POISONED.append(f"{what}: worker timed out")
        pytest.fail(f"{what}: worker timed out", pytrace=False)
    if r.returncode < 0 or r.returncode in (134, 139) \
            or "illegal memory access" in r.stderr:
        _GPU_POISONED.append(f"{what}: worker exit {r.returncode}")
    assert r.returncode == 0, f"{what}: exit {r.returncode}\n{r.stderr[-2000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"cases"')]
    assert len(lines) == 1, r.stdout[-2000:]
    got = {c["id"]: c for c in json.loads(lines[0])["cases"]}
    cases = _exact.config_cases(knobs)
    assert set(got) == {_exact.case_id(c) for c in cases}
    seen = set()
    for c in cases:
        res = got[_exact.case_id(c)]
        _assert_result(res, f"{what} {_exact.case_id(c)}")
        assert res["cfg"] == _exact.expected_config(knobs, c), \
            f"{what} {_exact.case_id(c)}: ran {res['cfg']}"
        seen.add((res["cfg"]["is_fp32"], res["cfg"]["beta_one"],
                  res["cfg"]["bk"], res["cfg"]["bm"]))
    # the variant under test really ran, for every type x beta it has
    # (and its fallbacks too, so a typo in a knob cannot pass vacuously)
    cfg = knobs.get("MARLIN_GEMM_CFG", "")
    for beta in (0, 1):
        if cfg == "bk32":
            assert {(0, beta, 32, 128), (1, beta, 32, 128),
                    (0, beta, 16, 128), (1, beta, 16, 128)} <= seen
        elif cfg == "bm256":
            assert {(0, beta, 16, 256), (0, beta, 16, 128),
                    (1, beta, 16, 128)} <= seen
            assert not any(s[0] == 1 and s[3] == 256 for s in seen)


# ---------------------------------------------------------------------------
# argument guards: every call below is rejected on the host before any
# kernel launch (mxk_gemm / mxk_sgemm_tn_epilogue return -4 ahead of
# their hipLaunchKernelGGL), so the tiny buffers are never touched.
def _gemm_rc(eng, d, fp32, m, k, n, lda, ldb, ldc, beta=0):
    return E.lib().mx_gemm_device_ex(eng._ctx, fp32, beta, m, k, n, d, lda,
                                     d, ldb, d, ldc)


def _epi_rc(eng, d, m, k, n, lda, ldb, ldc, add=None):
    return E.lib().mx_sgemm_epilogue_device(eng._ctx, m, k, n, d, lda, d,
                                            ldb, d, ldc, add)


def test_gemm_argument_guards(eng):
    _require_healthy()
    EINVAL = -4
    d = eng.alloc(64)
    try:
        for fp32, e16 in ((0, 2), (1, 4)):
            m, k, n = 256, 32, 128
            good = (m, k, m)
            # pitch smaller than the leading dimension
            assert _gemm_rc(eng, d, fp32, m, k, n, m - e16, k, m) == EINVAL
            assert _gemm_rc(eng, d, fp32, m, k, n, m, k - e16, m) == EINVAL
            assert _gemm_rc(eng, d, fp32, m, k, n, m, k, m - e16) == EINVAL
            assert _gemm_rc(eng, d, fp32, m, k, n, 0, k, m) == EINVAL
            assert _gemm_rc(eng, d, fp32, m, k, n, m, k, -m) == EINVAL
            # pitch that breaks 16-byte column alignment
            for off in range(1, e16):
                assert _gemm_rc(eng, d, fp32, m, k, n, m + off, k, m) == EINVAL
                assert _gemm_rc(eng, d, fp32, m, k, n, m, k + off, m) == EINVAL
                assert _gemm_rc(eng, d, fp32, m, k, n, m, k, m + off) == EINVAL
                assert _gemm_rc(eng, d, fp32, m, k, n, m, k, m + off,
                                beta=1) == EINVAL
            # k == 0 would memset through ldc: bad ldc rejected first
            assert _gemm_rc(eng, d, fp32, m, 0, n, m, 0, m - e16) == EINVAL
            # unpadded / negative dims (pre-existing checks)
            assert _gemm_rc(eng, d, fp32, m + 1, k, n, *good) == EINVAL
            assert _gemm_rc(eng, d, fp32, m, k + 1, n, *good) == EINVAL
            assert _gemm_rc(eng, d, fp32, m, k, n + 1, *good) == EINVAL
            assert _gemm_rc(eng, d, fp32, -128, k, n, *good) == EINVAL
            # the documented no-op stays a no-op (nothing launched)
            assert _gemm_rc(eng, d, fp32, 0, k, n, 0, k, 0) == 0
        # fp64 accepts an even pitch that fp32 must reject
        assert _gemm_rc(eng, d, 1, 256, 32, 128, 258, 32, 256) == EINVAL
    finally:
        eng.free(d)


@pytest.mark.parametrize("beta", [0, 1], ids=["b0", "b1"])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_gemm_k_zero_effect(eng, fp32, beta):
    # k == 0 launches no kernel: C = 0 is a 2-D memset of the M x N
    # interior through pitch ldc (pad rows and the trailing column keep
    # their bits), C += 0 touches nothing. C is prefilled as in
    # run_gemm_case.
    _require_healthy()
    import numpy as np
    M, N = 256, 128
    ldc = M + _exact.PAD
    dt = _exact.dtype_of(fp32)
    c = _exact.Case(fp32, beta, M, N, 16)
    nan = _exact._nan(dt)
    sentinel = dt(_exact.FINITE_SENTINEL) if beta else nan
    cimg = (_exact._padded(_exact.gemm_inputs(c)[2], ldc, 1, sentinel) if beta
            else _exact._filled(ldc, N + 1, nan))
    bufs = []
    try:
        d = eng.alloc(64)               # A and B: never read at k == 0
        bufs.append(d)
        dC = _exact._dev(eng, cimg, bufs)
        rc = E.lib().mx_gemm_device_ex(eng._ctx, fp32, beta, M, 0, N, d,
                                       M + _exact.PAD, d, _exact.PAD, dC, ldc)
        if rc == -2:
            _GPU_POISONED.append("k == 0: HIP runtime failure in-process")
        assert rc == 0
        got = np.empty_like(cimg)
        eng.download(got, dC, got.nbytes)
    finally:
        for b in bufs:
            eng.free(b)
    gbits, cbits = _exact._bits(got), _exact._bits(cimg)
    if beta:
        assert (gbits == cbits).all()
    else:
        assert (gbits[:M, :N] == 0).all()            # exactly +0.0
        sbits = sentinel.view(_exact.UINT[dt])
        assert (gbits[M:, :] == sbits).all()
        assert (gbits[:, N:] == sbits).all()


def test_epilogue_argument_guards(eng):
    _require_healthy()
    EINVAL = -4
    d = eng.alloc(64)
    try:
        m, k, n = 128, 16, 256
        # C is n x m: ldc is bounded by n, not m
        assert _epi_rc(eng, d, m, k, n, m, k, n - 4) == EINVAL
        assert _epi_rc(eng, d, m, k, n, m, k, m) == EINVAL
        assert _epi_rc(eng, d, m, k, n, m - 4, k, n) == EINVAL
        assert _epi_rc(eng, d, m, k, n, m, k - 4, n) == EINVAL
        for off in (1, 2, 3):
            assert _epi_rc(eng, d, m, k, n, m, k, n + off) == EINVAL
            assert _epi_rc(eng, d, m, k, n, m, k, n + off, add=d) == EINVAL
            assert _epi_rc(eng, d, m, k, n, m + off, k, n) == EINVAL
            assert _epi_rc(eng, d, m, k, n, m, k + off, n) == EINVAL
        # empty shapes: no no-op on this entry (the kernel prefetches
        # k-tile 0 unconditionally; a zero grid is a launch error)
        assert _epi_rc(eng, d, m, 0, n, m, 16, n) == EINVAL
        assert _epi_rc(eng, d, 0, k, n, 128, k, n) == EINVAL
        assert _epi_rc(eng, d, m, k, 0, m, k, 128) == EINVAL
        assert _epi_rc(eng, d, -128, k, n, m, k, n) == EINVAL
        assert _epi_rc(eng, d, m, -16, n, m, k, n) == EINVAL
        assert _epi_rc(eng, d, m, k, -128, m, k, n) == EINVAL
    finally:
        eng.free(d)


def test_last_gemm_config_argument_check(eng):
    _require_healthy()
    assert E.lib().mx_last_gemm_config(eng._ctx, None) == -4
    assert E.lib().mx_last_gemm_config(None, ctypes.byref(E.MxGemmCfg())) == -4
