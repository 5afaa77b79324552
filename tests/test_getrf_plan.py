# The LU factorisation plan without a GPU: the argument check, the step
# list and the in-block elimination of marlin_amd/csrc/getrf_plan.h, driven
# by a stand-alone program (tests/data/getrf_plan_check.cpp) built under
# AddressSanitizer + UBSan with the runtimes linked statically into the
# program, so that it needs nothing from its environment. Where the
# toolchain cannot link the sanitizers the same program is built plain,
# with a warning in the test report: its own checks still run.
# The program compares every decision of the check with 128-bit arithmetic
# and EXECUTES the blocked sweep at block width 4 for every order 0 .. 13 in
# both element types on exact data (mx_getrf_eliminate, a plain-loop row
# permutation, substitutions staged through mx_trsm_stage, a plain-loop
# update), against the known factors and an unblocked elimination written
# there independently. Here its decisions are compared with the Python
# restatement the GPU tests use.
import os
import subprocess
import warnings

import pytest

import _getrf_cases as GC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "getrf_plan_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("getrf") / "getrf_plan_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        # not silently: the run below then proves less, and says so
        warnings.warn("getrf_plan_check built WITHOUT sanitizers, the "
                      "sanitizer link failed: " + r.stderr[-300:])
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout.splitlines()


def test_getrf_plan_under_asan(report):
    assert report[-1].startswith("getrf_plan OK "), report[-5:]
    assert int(report[-1].split()[2]) > 50000
    # every order 0 .. 13 was executed in both types
    assert "check exec fp64 orders 14" in report
    assert "check exec fp32 orders 14" in report


def test_tie_and_zero_pivot_rows(report):
    # the lowest row of a tie; the first zero pivot, with the sweep finished
    assert report.count("check tie piv0 2 piv4 4") == 2
    assert report.count("check zero info 7") == 2


def test_check_restatement_agrees(report):
    rows = [ln.split()[1:] for ln in report if ln.startswith("decide ")]
    assert len(rows) == 16
    seen = set()
    for n, lda, ba, bp, rc, empty in (map(int, r) for r in rows):
        assert GC.check(4, 0, n, ba, lda, bp) == (rc, bool(empty)), \
            (n, lda, ba, bp)
        seen.add(rc)
    assert seen == {0, GC.EINVAL}       # both sides of the edge were shown


def test_check_restatement_edges():
    # n = 129 in fp64: the image is 256 x 256 at pitch 256, dPiv 1024 bytes
    full = 256 * 256 * 8
    assert GC.check(128, 0, 129, full, 256, 1024) == (0, False)
    assert GC.check(128, 0, 129, full - 1, 256, 1024)[0] == GC.EINVAL
    assert GC.check(128, 0, 129, full, 256, 1023)[0] == GC.EINVAL
    assert GC.check(128, 0, 129, full, 255, 1024)[0] == GC.EINVAL
    assert GC.check(128, 0, 129, full + 8 * 255, 257, 1024)[0] == GC.EINVAL
    assert GC.check(128, 0, -1, full, 256, 1024)[0] == GC.EINVAL
    assert GC.check(128, 2, 129, full, 256, 1024)[0] == GC.EINVAL
    assert GC.check(128, 0, 129, full, 256, 1024, info_null=True)[0] \
        == GC.EINVAL
    assert GC.check(128, 0, 0, 0, 0, 0) == (0, True)
    assert GC.check(128, 0, 2 ** 31, 2 ** 70, 2 ** 31, 2 ** 40)[0] == GC.EINVAL
