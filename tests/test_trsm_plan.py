# The triangular-solve plan without a GPU: the argument check, the step
# list and the diagonal-block staging of marlin_amd/csrc/trsm_plan.h, driven
# by a stand-alone program (tests/data/trsm_plan_check.cpp) built under
# AddressSanitizer + UBSan with the runtimes linked statically into the
# program, so that it needs nothing from its environment. Where the
# toolchain cannot link the sanitizers the same program is built plain,
# with a warning in the test report: its own checks still run.
# The program compares every decision of the check with 128-bit arithmetic
# and EXECUTES the plan at block width 4 (naive diagonal solve through the
# kernel's staging function, naive GEMM) for all 16 forms on exact data
# with NaN in everything that must not be read. Here its decisions are
# compared with the Python restatement the GPU tests use.
import os
import subprocess
import warnings

import pytest

import _trsm_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "trsm_plan_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trsm") / "trsm_plan_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        # not silently: the run below then proves less, and says so
        warnings.warn("trsm_plan_check built WITHOUT sanitizers, the "
                      "sanitizer link failed: " + r.stderr[-300:])
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout.splitlines()


def test_trsm_plan_under_asan(report):
    assert report[-1].startswith("trsm_plan OK "), report[-5:]
    assert int(report[-1].split()[2]) > 100000
    # 16 forms x 8 orders x 2 right-hand-side counts were executed
    assert "check exec cases 256" in report


def test_check_restatement_agrees(report):
    rows = [ln.split()[1:] for ln in report if ln.startswith("decide ")]
    assert len(rows) == 8
    seen = set()
    for n, r, ldt, ldb, bt, bb, rc, empty in (map(int, r) for r in rows):
        assert TC.check(4, 0, 0, 1, 0, 0, n, r, bt, ldt, bb, ldb) == (
            rc, bool(empty)), (n, r, ldt, ldb, bt, bb)
        seen.add(rc)
    assert seen == {0, TC.EINVAL}       # both sides of the edge were shown


def test_sweep_direction_restatement_agrees(report):
    rows = [ln.split() for ln in report if ln.startswith("steps ")]
    assert len(rows) == 8               # (side, lower, trans) at n = 9, w = 4
    for row in rows:
        side, lower, trans, n = map(int, row[1:5])
        steps = [tuple(map(int, s.split("/"))) for s in row[6:]]
        j0 = [s[0] for s in steps]
        fwd = TC.sweep_forward(side, lower, trans)
        assert j0 == ([0, 4, 8] if fwd else [8, 4, 0]), row
        # the rest is what lies ahead in the direction of the sweep
        for j, rest0, rest_len in steps:
            assert (rest0, rest_len) == ((j + 4, 12 - j - 4) if fwd
                                         else (0, j)), row
