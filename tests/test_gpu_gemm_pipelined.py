# The pipelined one-barrier k-loop of gemm_mfma_kernel against the
# two-barrier loop it replaces (MARLIN_GEMM_LOOP=twobar):
#   - exact-integer products (tests/_exact.py) at the tile counts and
#     knobs the existing table does not reach -- 4 tiles, the longest
#     provably exact K, bk32 / bm256 / phase rotation at long K -- under
#     the per-variant default and both forced loops (=twobar, =pipe),
#     each asserting the loop that actually ran;
#   - raw-bit identity of the two loops on non-integer data, which pins
#     the accumulation order (integer data is exact in any order).
# Knobs are latched per process: every run is a fresh child
# (gemm_loop_worker.py) with its own timeout.
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact
import _pipelined_cases as PC
from marlin_amd import Engine
from marlin_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_loop_worker.py")

# Once a GPU process of this module has faulted, timed out or died by a
# signal, nothing further is started on the device: every remaining test
# fails immediately with the first failure's reason.
_GPU_POISONED = []


def _require_healthy():
    if _GPU_POISONED:
        pytest.fail("not run: an earlier GPU process of this module "
                    f"failed hard ({_GPU_POISONED[0]})", pytrace=False)


def _run_worker(what, knobs, *args):
    """One child with exactly `knobs` set; returns its JSON record."""
    _require_healthy()
    env = {k: v for k, v in os.environ.items() if k not in PC.KNOBS}
    env.update(knobs)
    try:
        r = subprocess.run([sys.executable, WORKER, *args], env=env,
                           timeout=120, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _GPU_POISONED.append(f"{what}: worker timed out")
        pytest.fail(f"{what}: worker timed out", pytrace=False)
    if r.returncode < 0 or r.returncode in (134, 139) \
            or "illegal memory access" in r.stderr:
        _GPU_POISONED.append(f"{what}: worker exit {r.returncode}")
    assert r.returncode == 0, f"{what}: exit {r.returncode}\n{r.stderr[-2000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _assert_result(res, what):
    if res["rc"] == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure in worker")
    assert res["rc"] == 0, f"{what}: entry returned {res['rc']}"
    assert res["ok"], f"{what}: first mismatch at (row, col) {res['first_bad']}"
    assert not res["sentinel_inside"], f"{what}: sentinel left inside C"
    assert res["pad_ok"], f"{what}: pad rows / trailing column overwritten"


# ---------------------------------------------------------------------------
# exact-integer cases, every variant under both loops
@pytest.mark.parametrize("loop", list(PC.LOOPS))
@pytest.mark.parametrize("variant", list(PC.VARIANTS))
def test_gemm_exact_both_loops(variant, loop):
    knobs = dict(PC.VARIANTS[variant], **PC.LOOPS[loop])
    what = f"{variant}/{loop}"
    got = {c["id"]: c for c in
           _run_worker(what, knobs, "exact", variant)["cases"]}
    cases = PC.exact_cases(variant)
    assert set(got) == {_exact.case_id(c) for c in cases}
    seen = set()
    for c in cases:
        res = got[_exact.case_id(c)]
        cid = f"{what} {_exact.case_id(c)}"
        _assert_result(res, cid)
        assert res["cfg"] == _exact.expected_config(knobs, c), \
            f"{cid}: ran {res['cfg']}"
        # the loop the environment asked for really ran (a mistyped knob
        # would leave the default loop running and fail here)
        assert res["loop"] == PC.expected_loop(loop, res["cfg"]), \
            f"{cid}: ran loop {res['loop']}"
        seen.add((res["cfg"]["is_fp32"], res["cfg"]["beta_one"],
                  res["cfg"]["bk"], res["cfg"]["bm"]))
    for beta in (0, 1):
        if variant == "bk32":
            assert {(0, beta, 32, 128), (1, beta, 32, 128)} <= seen
        elif variant == "bm256":
            # 512 rows run the 256-row tile, 384 rows fall back; fp32 has
            # no 256-row instantiation
            assert {(0, beta, 16, 256), (0, beta, 16, 128),
                    (1, beta, 16, 128)} <= seen
        else:
            assert seen == {(f, b, 16, 128) for f in (0, 1) for b in (0, 1)}


# ---------------------------------------------------------------------------
# bit-identity of the two loops on non-integer data
@pytest.fixture(scope="module")
def bits_runs(tmp_path_factory):
    """{loop: (records by id, directory of C images)}, one child each."""
    out = {}
    for loop, knobs in PC.LOOPS.items():
        d = tmp_path_factory.mktemp(f"bits_{loop}")
        recs = _run_worker(f"bits/{loop}", knobs, "bits", str(d))["bits"]
        out[loop] = ({r["id"]: r for r in recs}, d)
    return out


@pytest.mark.parametrize("fp32,beta", PC.BITS_CASES,
                         ids=[PC.bits_id(*c) for c in PC.BITS_CASES])
def test_loops_bit_identical_on_random_data(bits_runs, fp32, beta):
    cid = PC.bits_id(fp32, beta)
    cfg = {"is_fp32": fp32, "bk": 16}        # no MARLIN_GEMM_CFG here
    imgs = {}
    for loop, (recs, d) in bits_runs.items():
        assert cid in recs, f"{cid}/{loop}: not run"
        assert recs[cid]["rc"] == 0, f"{cid}/{loop}: rc {recs[cid]['rc']}"
        assert recs[cid]["loop"] == PC.expected_loop(loop, cfg), \
            f"{cid}/{loop}: ran loop {recs[cid]['loop']}"
        imgs[loop] = np.load(os.path.join(d, cid + ".npy"))
    ref = imgs["twobar"]
    m, n, _ = PC.BITS_SHAPE
    assert ref.shape == (m, n) and ref.dtype == _exact.dtype_of(fp32)
    # a real product, not equal blanks: entries of A, B are U[0,1), so
    # every element of A*B is positive and finite
    assert np.isfinite(ref).all() and (ref > 0).all()
    uref = ref.view(_exact.UINT[ref.dtype.type])
    for loop in ("pipe", "default"):
        got = imgs[loop]
        assert got.shape == ref.shape and got.dtype == ref.dtype
        bad = np.argwhere(got.view(uref.dtype) != uref)
        assert len(bad) == 0, (f"{cid}/{loop}: {len(bad)} elements differ "
                               f"from twobar, first at {bad[0].tolist()}")


# ---------------------------------------------------------------------------
def test_last_gemm_loop_argument_check():
    _require_healthy()
    import ctypes
    eng = Engine(0)
    try:
        assert E.lib().mx_last_gemm_loop(eng._ctx, None) == -4
        assert E.lib().mx_last_gemm_loop(None, ctypes.byref(ctypes.c_int())) == -4
        assert eng.last_gemm_loop() in (0, 1)
    finally:
        eng.close()
