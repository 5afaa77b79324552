# Exact-arithmetic tests of the SUMMA panel loop (summa_loop / pack_panel
# in marlin_gpu.cpp) at every position of several grids, on one GPU.
#
# One device cannot host two RCCL ranks, so the multi-rank positions run
# through mx_gemm_summa_virtual: the same loop, pack, k-padding, double
# buffering, events and accumulate chain as the real entries, with each
# panel packed from its root's shard instead of broadcast. What stays
# unpinned is exactly that replaced step: the ncclBroadcast roots and
# counts on a real multi-GPU grid.
#
# Inputs are exact (tests/_exact_summa.py), so every comparison is exact
# equality: the logical block, no sentinel left inside, pad rows and pad
# columns of C_local exactly zero, guard column untouched, and
# gemm_launches equal to the planned panel count.
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact
import _exact_summa as S
from marlin_amd import Engine
from marlin_amd import engine as E

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "summa_worker.py")

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


def _assert_result(res, what, launches):
    if res["rc"] == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure in-process")
    assert res["rc"] == 0, f"{what}: entry returned {res['rc']}"
    assert res["ok"], f"{what}: first mismatch at (row, col) {res['first_bad']}"
    assert not res["sentinel_inside"], f"{what}: sentinel left inside C"
    assert res["pad_rows_zero"], f"{what}: C_local pad rows not zero"
    assert res["pad_cols_zero"], f"{what}: C_local pad columns not zero"
    assert res["pad_ok"], f"{what}: guard column overwritten"
    assert res["launches"] == launches, \
        f"{what}: {res['launches']} GEMM launches, plan has {launches}"
    assert res["comm_ms"] == 0, f"{what}: comm_ms {res['comm_ms']}"


def _assert_case(results, c):
    assert set(results) == {(i, j) for i in range(c.pr) for j in range(c.pc)}
    for (prow, pcol), res in sorted(results.items()):
        _assert_result(res, f"{S.case_id(c)} at ({prow},{pcol})",
                       S.expected_launches(c, prow, pcol))


# ---------------------------------------------------------------------------
# a. virtual ranks, every position of every grid
@pytest.mark.parametrize("case", S.virtual_cases(), ids=S.case_id)
def test_summa_virtual_exact(eng, case):
    _require_healthy()
    _assert_case(S.run_virtual_case(eng, case), case)


def test_summa_virtual_argument_checks(eng):
    # every call below is rejected before anything is enqueued
    _require_healthy()
    EINVAL = -4
    d = eng.alloc(64)
    try:
        one = (ctypes.c_void_p * 1)(d)
        two = (ctypes.c_void_p * 2)(d, d)

        def rc(pr, pc, prow, pcol, arow, bcol, dC, m=256, k=64, n=256, kb=0):
            return E.lib().mx_gemm_summa_virtual(
                eng._ctx, 0, pr, pc, prow, pcol, m, k, n, arow, bcol, dC, kb)
        assert rc(0, 1, 0, 0, one, one, d) == EINVAL
        assert rc(1, 0, 0, 0, one, one, d) == EINVAL
        assert rc(2, 1, 2, 0, one, two, d) == EINVAL
        assert rc(2, 1, -1, 0, one, two, d) == EINVAL
        assert rc(1, 2, 0, 2, two, one, d) == EINVAL
        assert rc(1, 1, 0, 0, None, one, d) == EINVAL
        assert rc(1, 1, 0, 0, one, None, d) == EINVAL
        assert rc(1, 1, 0, 0, one, one, None) == EINVAL
        assert rc(1, 1, 0, 0, one, one, d, kb=-16) == EINVAL
        # a non-empty shard of the row / column is missing
        assert rc(2, 1, 0, 0, one, (ctypes.c_void_p * 2)(d, None),
                  d) == EINVAL
        assert rc(1, 2, 0, 0, (ctypes.c_void_p * 2)(None, d), one,
                  d) == EINVAL
        assert E.lib().mx_gemm_summa_virtual(
            None, 0, 1, 1, 0, 0, 256, 64, 256, one, one, d, 0) == EINVAL
    finally:
        eng.free(d)


# ---------------------------------------------------------------------------
# b. stale pad columns of the B panel buffer
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_summa_b_panel_pad_columns_zeroed(fp32):
    # An aligned panel (kb % 16 == 0) skips the whole-buffer memset, and
    # the B pack copies nj columns only: columns nj..njp of the panel
    # buffer must be zeroed by the pack itself. Step 1 leaves NaN in all
    # 256 columns of both panel buffers of a fresh engine (nj = 256 is a
    # multiple of 128, B all NaN); step 2 reuses the same buffers at the
    # same pitch (kb = 64) with nj = 200 < njp = 256.
    _require_healthy()
    dt = _exact.dtype_of(fp32)
    eng = Engine(0)
    bufs = []
    try:
        m, k, n, kb = 128, 128, 256, 64
        dA = _exact._dev(eng, np.zeros((m, k), dtype=dt, order="F"), bufs)
        dB = _exact._dev(eng, _exact._filled(k, n, _exact._nan(dt)), bufs)
        dC = _exact._dev(eng, np.zeros((m, n), dtype=dt, order="F"), bufs)
        eng.gemm_summa_virtual(1, 1, 0, 0, m, k, n, [dA], [dB], dC, kb,
                               bool(fp32))
        assert eng.stats()["gemm_launches"] == 2
        poisoned = np.empty((m, n), dtype=dt, order="F")
        eng.download(poisoned, dC, poisoned.nbytes)
        assert np.isnan(poisoned).all()      # the NaN really went through
        c = S.SummaCase(fp32, 1, 1, 256, 512, 200, kb)
        assert all((k1 - k0) % 16 == 0
                   for k0, k1, _, _ in E.plan_panels(c.k, 1, 1, kb))
        results = S.run_virtual_case(eng, c)
    except E.EngineError as e:
        if e.code == -2:
            _GPU_POISONED.append("pad-column regression: HIP failure")
        raise
    finally:
        for d in bufs:
            eng.free(d)
        eng.close()
    _assert_case(results, c)


# ---------------------------------------------------------------------------
# c. real one-rank entries, in-process
def _default_kb():
    return int(os.environ.get("MARLIN_SUMMA_KB", "0") or 0) or 2048


@pytest.fixture(scope="module")
def comm_eng(eng):
    eng.comm_init(0, 1, Engine.comm_id())
    return eng


@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_summa_real_one_rank_entries(comm_eng, fp32):
    _require_healthy()
    eng = comm_eng
    assert eng.grid() == (1, 1, 0, 0)
    c = S.SummaCase(fp32, 1, 1, *S.REAL_SHAPES[fp32], _default_kb())
    npan = len(E.plan_panels(c.k, 1, 1, c.kb))
    if not fp32 and c.kb == 2048:
        assert npan == 2
    # virtual (1,1,0,0) on the same shards, default width (kb_max = 0)
    virt = []
    res = S.run_virtual_case(eng, c, keep=virt, kb_arg=0)
    _assert_case(res, c)
    vbits = _exact._bits(virt[0])
    # panel-loop device entry
    real = []
    res = S.run_real_device(eng, c, "summa", keep=real)
    _assert_result(res, f"{S.case_id(c)} summa_device", npan)
    assert (_exact._bits(real[0]) == vbits).all()
    # k-resident device entry: one GEMM over the whole k
    kres = []
    res = S.run_real_device(eng, c, "kres", keep=kres)
    _assert_result(res, f"{S.case_id(c)} kres_device", 1)
    assert (_exact._bits(kres[0]) == vbits).all()
    # k-resident host entry (returns the logical block)
    host = []
    res = S.run_real_host(eng, c, "kres", keep=host)
    _assert_result(res, f"{S.case_id(c)} kres host", 1)
    assert (_exact._bits(host[0])
            == _exact._bits(virt[0][:c.m, :c.n])).all()


# ---------------------------------------------------------------------------
# d. real one-rank entries at MARLIN_SUMMA_KB=40, one fresh child
def test_summa_real_entries_kb_knob_child():
    _require_healthy()
    env = dict(os.environ, MARLIN_SUMMA_KB=str(S.KNOB_KB))
    what = f"MARLIN_SUMMA_KB={S.KNOB_KB}"
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
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"runs"')]
    assert len(lines) == 1, r.stdout[-2000:]
    got = {x["id"]: x for x in json.loads(lines[0])["runs"]}
    assert set(got) == {"f64-device", "f64-host", "f32-device", "f32-host"}
    npan = len(E.plan_panels(S.KNOB_SHAPE[1], 1, 1, S.KNOB_KB))
    assert npan == 13
    for rid, res in sorted(got.items()):
        _assert_result(res, f"{what} {rid}", npan)
