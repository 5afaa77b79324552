# The grouped GEMM entry (mx_gemm_device_grouped): many independent
# products in one launch.
#   1. exact-integer heterogeneous group (tests/_grouped_cases.SHAPES, 31
#      blocks) for both types, both betas and the four op forms, under each
#      forced k-loop: two fresh children (gemm_grouped_worker.py), one
#      after the other;
#   2. raw-bit identity with mx_gemm_device_op problem by problem on
#      ordinary data (same children), shared A, dA == dB, a group of one;
#   3. A, B and C as rectangles of one buffer (element offsets);
#   4. 1, then 300, then 2 problems on one context (table workspace);
#   5. degenerate calls and the stats / introspection they leave;
#   6. one minimal refused table per validation rule: host-side refusals,
#      no table the validation would refuse ever reaches the kernel.
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _exact
import _grouped_cases as GC
from marlin_amd import Engine

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "gemm_grouped_worker.py")
EINVAL = -4

# Once a GPU process of this module has faulted, timed out or died by a
# signal, nothing further is started on the device: every remaining test
# fails immediately with the first failure's reason.
_GPU_POISONED = []


def _require_healthy():
    if _GPU_POISONED:
        pytest.fail("not run: an earlier GPU process of this module "
                    f"failed hard ({_GPU_POISONED[0]})", pytrace=False)


def _run_worker(loop):
    _require_healthy()
    env = {k: v for k, v in os.environ.items() if k not in GC.KNOBS}
    env.update(GC.LOOPS[loop])
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


@pytest.fixture(scope="module")
def runs():
    """{loop: worker record}: the two children, one after the other."""
    return {loop: _run_worker(loop) for loop in GC.LOOPS}


@pytest.fixture(scope="module")
def eng():
    _require_healthy()
    e = Engine(0)
    yield e
    e.close()


def _rc_ok(rec, what):
    if rec["rc"] == -2:
        _GPU_POISONED.append(f"{what}: HIP runtime failure")
    assert rec["rc"] == 0, f"{what}: entry returned {rec['rc']}"


# ---------------------------------------------------------------------------
# 1. exact, heterogeneous
@pytest.mark.parametrize("loop", list(GC.LOOPS))
@pytest.mark.parametrize("fp32,beta,form", GC.COMBOS,
                         ids=[GC.combo_id(*c) for c in GC.COMBOS])
def test_grouped_exact_heterogeneous(runs, fp32, beta, form, loop):
    cid = GC.combo_id(fp32, beta, form)
    what = f"{cid}/{loop}"
    assert cid in runs[loop]["exact"], f"{what}: not run"
    rec = runs[loop]["exact"][cid]
    _rc_ok(rec, what)
    assert len(rec["problems"]) == len(GC.SHAPES)
    for shape, res in zip(GC.SHAPES, rec["problems"]):
        w = f"{what} {shape}"
        assert res["ok"], f"{w}: first mismatch at (row, col) {res['first_bad']}"
        assert not res["sentinel_inside"], f"{w}: sentinel left inside C"
        assert res["pad_ok"], f"{w}: pad rows / guard column overwritten"
    assert rec["group"] == [len(GC.SHAPES), GC.BLOCKS]
    assert rec["launches"] == 1
    assert rec["flops"] == GC.expected_flops(GC.SHAPES)
    # the launch is reported like any other: default geometry, phase 0,
    # the band of the first table entry (384 x 256 x 80: nbn = 2)
    assert rec["cfg"] == {"is_fp32": fp32, "beta_one": beta, "bk": 16,
                          "bm": 128, "waves": 4, "band": 2, "phase_mask": 0}
    assert rec["op"] == list(GC.FORMS[form])
    assert rec["loop"] == (1 if loop == "pipe" else 0)


# ---------------------------------------------------------------------------
# 2. bit-identity with the plain entry
@pytest.mark.parametrize("loop", list(GC.LOOPS))
@pytest.mark.parametrize("fp32,beta", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_grouped_bits_equal_plain_entry(runs, fp32, beta, loop):
    cid = GC.combo_id(fp32, beta, "nn")
    what = f"bits {cid}/{loop}"
    assert cid in runs[loop]["bits"], f"{what}: not run"
    rec = runs[loop]["bits"][cid]
    _rc_ok(rec, what)
    assert rec["real"], f"{what}: the plain results are not real products"
    assert len(rec["equal"]) == len(GC.SHAPES) + 2
    assert all(rec["equal"]), f"{what}: problems differ: {rec['equal']}"
    assert rec["group"] == [len(GC.SHAPES) + 2, GC.BLOCKS + 1 + 2]
    assert rec["one"], f"{what}: group of one differs from the plain entry"
    assert rec["one_group"] == [1, 6]
    assert rec["gram"], f"{what}: dA == dB under trans_a differs"
    assert rec["op"] == [1, 0]
    assert rec["loop"] == (1 if loop == "pipe" else 0)


# ---------------------------------------------------------------------------
# 3. offsets
@pytest.mark.parametrize("fp32", [0, 1])
def test_grouped_offsets_in_one_buffer(eng, fp32):
    _require_healthy()
    img, want, rows = GC.offsets_case(fp32)
    d = eng.alloc(img.nbytes)
    try:
        eng.upload(d, img, img.nbytes)
        rc = eng.gemm_grouped_raw(rows(d), fp32, accumulate=True, check=False)
        _rc_ok({"rc": rc}, "offsets")
        got = np.empty_like(img)
        eng.download(got, d, got.nbytes)
    finally:
        eng.free(d)
    assert eng.last_gemm_group() == (4, 4)
    # the default loop of each type (no knob here)
    assert eng.last_gemm_loop() == (0 if fp32 else 1)
    U = _exact.UINT[img.dtype.type]
    # the four C blocks really changed, and nothing else did
    assert not (want.view(U) == img.view(U)).all()
    np.testing.assert_array_equal(got.view(U), want.view(U))


# ---------------------------------------------------------------------------
# 4. many problems, workspace growth
def test_grouped_many_problems_and_workspace_growth(eng):
    _require_healthy()
    a, b = GC.many_inputs()
    nan = _exact._nan(np.float64)
    bufs = []
    try:
        dA = _exact._dev(eng, _exact._padded(a, 128 + _exact.PAD, 0, nan), bufs)
        dB = _exact._dev(eng, _exact._padded(b, 48 + _exact.PAD, 0, nan), bufs)
        for idxs, group in (([5], (1, 1)),
                            (list(range(GC.MANY)), (GC.MANY, GC.MANY)),
                            ([7, 2], (2, 2))):
            rc, same = GC.run_many(eng, dA, dB, a, b, idxs)
            _rc_ok({"rc": rc}, f"{len(idxs)} problems")
            assert same, f"{len(idxs)} problems: C image differs"
            assert eng.last_gemm_group() == group
            st = eng.stats()
            assert st["gemm_launches"] == 1
            assert st["flops"] == float(sum(
                2 * 128 * 128 * GC.many_problem(i)[0] for i in idxs))
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# 5. degenerate calls
def _small(eng, bufs, fill=None):
    """A 128 x 16, B 16 x 128 exact, C 128 x 128 of `fill` (NaN sentinel
    by default), tight pitches."""
    c = _exact.Case(0, 0, 128, 128, 16)
    a, b, _, ref = _exact.gemm_inputs(c)
    cimg = _exact._filled(128, 128, _exact._nan(np.float64)) if fill is None \
        else np.asfortranarray(np.full((128, 128), fill))
    return (_exact._dev(eng, a, bufs), _exact._dev(eng, b, bufs),
            _exact._dev(eng, cimg, bufs), cimg, ref)


def _fetch(eng, d, like):
    got = np.empty_like(like)
    eng.download(got, d, got.nbytes)
    return got


def test_grouped_degenerate_calls(eng):
    _require_healthy()
    bufs = []
    U = np.uint64
    try:
        dA, dB, dC, cimg, ref = _small(eng, bufs)
        r = GC.row
        # a real launch first, so "most recent grouped launch" is known
        assert eng.gemm_grouped_raw([r(128, 16, 128, dA, 0, 128, dB, 0, 16,
                                       dC, 0, 128)], check=False) == 0
        np.testing.assert_array_equal(_fetch(eng, dC, cimg), ref)
        assert eng.last_gemm_group() == (1, 1)
        eng.upload(dC, cimg, cimg.nbytes)

        def nothing_launched(rows, **kw):
            assert eng.gemm_grouped_raw(rows, check=False, **kw) == 0
            st = eng.stats()
            assert st["gemm_launches"] == 0 and st["gemm_ms"] == 0
            assert eng.last_gemm_group() == (1, 1)    # the launch above
            return st
        # count == 0, with and without a table
        assert nothing_launched([])["flops"] == 0
        assert nothing_launched(None)["flops"] == 0
        # every problem empty; an empty problem may carry NULL buffers
        st = nothing_launched([r(0, 16, 128, dA, 0, 128, dB, 0, 16, dC, 0, 128),
                               r(128, 16, 0, None, 0, 0, None, 0, 0, None, 0, 0),
                               r(0, 0, 0, dA, 0, 128, dB, 0, 16, dC, 0, 128)])
        assert st["flops"] == 0
        np.testing.assert_array_equal(_fetch(eng, dC, cimg).view(U),
                                      cimg.view(U))
        # k == 0 alone: nothing launched; C unchanged when accumulating,
        # zero otherwise
        k0 = [r(128, 0, 128, dA, 0, 128, dB, 0, 16, dC, 0, 128)]
        nothing_launched(k0, accumulate=True)
        np.testing.assert_array_equal(_fetch(eng, dC, cimg).view(U),
                                      cimg.view(U))
        nothing_launched(k0)
        assert not _fetch(eng, dC, cimg).view(U).any()
        # a mixture: m = 0, n = 0, k = 0 and one real problem, both betas
        for beta in (0, 1):
            seven = np.float64(7.0)
            dA2, dB2, dK, kimg, _ = _small(eng, bufs, seven)
            _, _, dM, mimg, _ = _small(eng, bufs)
            _, _, dR, rimg, _ = _small(eng, bufs, seven)
            rows = [r(0, 16, 128, dA, 0, 128, dB, 0, 16, dM, 0, 128),
                    r(128, 0, 128, dA, 0, 128, dB, 0, 16, dK, 0, 128),
                    r(128, 16, 0, dA, 0, 128, dB, 0, 16, dM, 0, 128),
                    r(128, 16, 128, dA2, 0, 128, dB2, 0, 16, dR, 0, 128)]
            assert eng.gemm_grouped_raw(rows, accumulate=bool(beta),
                                        check=False) == 0
            st = eng.stats()
            assert st["gemm_launches"] == 1
            assert st["flops"] == 2.0 * 128 * 16 * 128
            assert eng.last_gemm_group() == (1, 1)
            np.testing.assert_array_equal(_fetch(eng, dM, mimg).view(U),
                                          mimg.view(U))
            np.testing.assert_array_equal(_fetch(eng, dK, kimg),
                                          kimg if beta else 0 * kimg)
            np.testing.assert_array_equal(_fetch(eng, dR, rimg),
                                          ref + (7.0 if beta else 0.0))
    finally:
        for d in bufs:
            eng.free(d)


# ---------------------------------------------------------------------------
# 6. rejections
def test_grouped_rejections_touch_nothing(eng):
    _require_healthy()
    bufs = []
    U = np.uint64
    try:
        dA, dB, dC, cimg, _ = _small(eng, bufs)
        nan = _exact._nan(np.float64)
        big = _exact._filled(256, 256, nan)          # one 256-pitch image
        dI = _exact._dev(eng, big, bufs)
        r = GC.row
        ok = r(128, 16, 128, dA, 0, 128, dB, 0, 16, dC, 0, 128)

        def sub(**kw):
            names = ["m", "k", "n", "dA", "a_off", "lda", "dB", "b_off",
                     "ldb", "dC", "c_off", "ldc"]
            q = dict(zip(names, ok))
            q.update(kw)
            return tuple(q[n] for n in names)
        in_img = sub(dC=dI, ldc=256)                 # C = block (0, 0) of dI
        tables = {
            "m not a multiple of 128": [sub(m=64)],
            "n not a multiple of 128": [sub(n=192)],
            "k not a multiple of 16": [sub(k=8)],
            "negative m": [sub(m=-128)],
            "lda below m": [sub(lda=126)],
            "ldb below k": [sub(ldb=14)],
            "ldc below m": [sub(ldc=126)],
            "lda not a multiple of 16 bytes": [sub(lda=129)],
            "c_off not a multiple of 16 bytes": [sub(dC=dI, c_off=1, ldc=256)],
            "negative a_off": [sub(a_off=-2)],
            "NULL A": [sub(dA=None)],
            "NULL B": [sub(dB=None)],
            "NULL C": [sub(dC=None)],
            "NULL C with k == 0": [sub(dC=None, k=0)],
            "C one element past its buffer": [sub(c_off=2)],
            "A one column past its buffer": [sub(a_off=128)],
            "B past its buffer by its pitch": [sub(ldb=18)],
            "the same C twice": [ok, ok],
            "C rectangles one row overlapping": [in_img,
                                                 sub(dC=dI, c_off=126, ldc=256)],
            "C spans crossing, pitches differ": [in_img,
                                                 sub(dC=dI, c_off=128, ldc=254)],
            "C is also its own A": [sub(dA=dI, lda=256, dC=dI, ldc=256)],
            "C is another problem's B": [in_img, sub(dB=dI, ldb=256)],
            "a refused problem behind a legal one": [ok, sub(dC=dI, ldc=256,
                                                            k=24)],
        }
        for what, rows in tables.items():
            assert eng.gemm_grouped_raw(rows, check=False) == EINVAL, what
            assert eng.stats()["gemm_launches"] == 0, what
        # the nearest legal neighbours of the aliasing tables pass the
        # validation (they are launched: row-adjacent C rectangles)
        assert eng.gemm_grouped_raw(
            [in_img, sub(dC=dI, c_off=128, ldc=256)], check=False) == 0
        eng.upload(dI, big, big.nbytes)
        # the call as a whole
        for what, call in {
            "count < 0": lambda: eng._grouped_call(
                -1, None, False, False, 0, 0, check=False),
            "NULL problems with count > 0": lambda: eng._grouped_call(
                1, None, False, False, 0, 0, check=False),
            "trans_a = 2": lambda: eng.gemm_grouped_raw(
                [ok], trans_a=2, check=False),
            "trans_b = -1": lambda: eng.gemm_grouped_raw(
                [ok], trans_b=-1, check=False),
        }.items():
            assert call() == EINVAL, what
            assert eng.stats()["gemm_launches"] == 0, what
        # no refusal wrote anything
        for d, img in ((dC, cimg), (dI, big)):
            np.testing.assert_array_equal(_fetch(eng, d, img).view(U),
                                          img.view(U))
    finally:
        for d in bufs:
            eng.free(d)


def test_last_gemm_group_argument_check(eng):
    _require_healthy()
    import ctypes
    from marlin_amd import engine as E
    n, b = ctypes.c_int(), ctypes.c_int64()
    lib = E.lib()
    assert lib.mx_last_gemm_group(None, ctypes.byref(n), ctypes.byref(b)) == -4
    assert lib.mx_last_gemm_group(eng._ctx, None, ctypes.byref(b)) == -4
    assert lib.mx_last_gemm_group(eng._ctx, ctypes.byref(n), None) == -4
