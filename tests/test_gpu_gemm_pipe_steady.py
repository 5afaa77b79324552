# The steady-state body of the pipelined k-loop at short tile counts
# (tests/_pipe_steady_cases.py): 6, 7, 8 and 9 tiles, where the body runs
# 4 .. 7 times before the two peeled steps -- few enough that a step
# dropped, repeated or reading the wrong buffer at either parity, or a
# phase wrap of the running DMA pointers at the wrong tile, changes the
# result, which the long-K tables (65, 256 tiles) check only in bulk.
#   - exact-integer products (tests/_exact.py), fp64 and fp32, beta 0 and
#     1, under the default loop, under MARLIN_GEMM_LOOP=pipe and under the
#     MARLIN_GEMM_PHASE rotations, plus one TN, NT and TT product and one
#     grouped launch at 7 tiles, each asserting the loop that ran;
#   - raw-bit identity with the two-barrier loop on non-integer data.
# Knobs are latched per process: every run is a fresh child
# (gemm_pipe_steady_worker.py) with its own timeout.
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact
import _exact_op as XO
import _pipe_steady_cases as SC
import _pipelined_cases as PC

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_pipe_steady_worker.py")

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
# exact-integer cases under every knob set
@pytest.mark.parametrize("run", list(SC.RUNS))
def test_steady_state_exact(run):
    knobs = SC.RUNS[run]
    loop = SC.loop_of(run)
    rec = _run_worker(run, knobs, "exact", "-")
    got = {c["id"]: c for c in rec["cases"]}
    cases = SC.exact_cases()
    assert set(got) == {_exact.case_id(c) for c in cases}
    for c in cases:
        cid = f"{run} {_exact.case_id(c)}"
        res = got[_exact.case_id(c)]
        _assert_result(res, cid)
        assert res["cfg"] == _exact.expected_config(knobs, c), \
            f"{cid}: ran {res['cfg']}"
        assert res["loop"] == PC.expected_loop(loop, res["cfg"]), \
            f"{cid}: ran loop {res['loop']}"
    # transposed forms: default geometry, the knob's phase mask
    ops = {r["id"]: r for r in rec["ops"]}
    assert set(ops) == {SC.op_id(f, c) for f, c in SC.OP_CASES}
    for form, c in SC.OP_CASES:
        cid = f"{run} {SC.op_id(form, c)}"
        res = ops[SC.op_id(form, c)]
        _assert_result(res, cid)
        ta, tb = XO.FORMS[form]
        assert res["op"] == [ta, tb], f"{cid}: ran op {res['op']}"
        assert res["cfg"] == XO.expected_config(knobs, c, ta, tb), \
            f"{cid}: ran {res['cfg']}"
        assert res["loop"] == PC.expected_loop(loop, res["cfg"]), \
            f"{cid}: ran loop {res['loop']}"
    # grouped launch: fp64, so pipelined under every knob set here
    grp = rec["group"]
    assert grp is not None, f"{run}: grouped launch not run"
    if grp["rc"] == -2:
        _GPU_POISONED.append(f"{run}: HIP runtime failure in grouped launch")
    assert grp["rc"] == 0, f"{run}: grouped entry returned {grp['rc']}"
    blocks = sum((m // 128) * (n // 128) for m, n, _ in SC.GROUP_SHAPES)
    assert grp["group"] == [len(SC.GROUP_SHAPES), blocks]
    assert grp["loop"] == 1
    assert len(grp["problems"]) == len(SC.GROUP_SHAPES)
    for shape, res in zip(SC.GROUP_SHAPES, grp["problems"]):
        _assert_result(dict(res, rc=0), f"{run} grouped {shape}")


# ---------------------------------------------------------------------------
# bit-identity of the loops on non-integer data
@pytest.fixture(scope="module")
def bits_runs(tmp_path_factory):
    """{loop: (records by id, directory of C images)}, one child each."""
    out = {}
    for loop in SC.BITS_LOOPS:
        d = tmp_path_factory.mktemp(f"steady_bits_{loop}")
        recs = _run_worker(f"bits/{loop}", PC.LOOPS[loop], "bits",
                           str(d))["bits"]
        out[loop] = ({r["id"]: r for r in recs}, d)
    return out


@pytest.mark.parametrize("fp32,beta,shape", SC.BITS_CASES,
                         ids=[SC.bits_id(*c) for c in SC.BITS_CASES])
def test_steady_state_bit_identical_to_twobar(bits_runs, fp32, beta, shape):
    cid = SC.bits_id(fp32, beta, shape)
    cfg = {"is_fp32": fp32, "bk": 16}        # no MARLIN_GEMM_CFG here
    imgs = {}
    for loop, (recs, d) in bits_runs.items():
        assert cid in recs, f"{cid}/{loop}: not run"
        assert recs[cid]["rc"] == 0, f"{cid}/{loop}: rc {recs[cid]['rc']}"
        assert recs[cid]["loop"] == PC.expected_loop(loop, cfg), \
            f"{cid}/{loop}: ran loop {recs[cid]['loop']}"
        imgs[loop] = np.load(os.path.join(d, cid + ".npy"))
    ref = imgs["twobar"]
    assert ref.shape == shape[:2] and ref.dtype == _exact.dtype_of(fp32)
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
