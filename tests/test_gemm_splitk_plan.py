# The split-K slicing policy without a GPU: slice lists and the auto rule
# of marlin_amd/csrc/gemm_splitk_plan.h, driven by a stand-alone program
# (tests/data/gemm_splitk_plan_check.cpp) built under AddressSanitizer +
# UBSan with the runtimes linked statically into the program, so that it
# needs nothing from its environment. Where the toolchain cannot link the
# sanitizers the same program is built plain, with a warning in the test
# report: its own checks still run.
# The program checks the properties (cover, evenness, clamp, one wave,
# slice depth, monotone in k, no overflow); here its every decision is
# compared with the Python restatement of tests/_splitk_cases.py, which
# the GPU tests use. The tuned constant is read from the program, never
# asserted.
import os
import subprocess
import warnings

import pytest

import _splitk_cases as SK

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "gemm_splitk_plan_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("splitk") / "splitk_plan_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        # not silently: the run below then proves less, and says so
        warnings.warn("gemm_splitk_plan_check built WITHOUT sanitizers, the "
                      "sanitizer link failed: " + r.stderr[-300:])
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout.splitlines()


def test_gemm_splitk_plan_under_asan(report):
    assert report[-1].startswith("gemm_splitk_plan OK "), report[-5:]
    assert int(report[-1].split()[2]) > 10000


def test_header_constant_is_what_the_restatement_reads(report):
    assert report[0].split()[:2] == ["const", "MX_SPLITK_MIN_KSTEPS"]
    assert int(report[0].split()[2]) == SK.min_ksteps() >= 1
    assert report[1].split()[:2] == ["const", "MX_SPLITK_FILL_DIV"]
    assert int(report[1].split()[2]) == SK.fill_div() >= 1


def test_auto_restatement_agrees_on_the_whole_sweep(report):
    rows = [ln.split()[1:] for ln in report if ln.startswith("auto ")]
    assert len(rows) == 2 * 4 * 8 * 8 * 11
    split = 0
    for fp32, m, n, k, cus, s in (map(int, r) for r in rows):
        assert SK.auto_slices(fp32, m, n, k, cus) == s, (fp32, m, n, k, cus)
        split += s > 1
    assert split > 100          # the sweep does reach the splitting branch


def test_slice_restatement_agrees_on_the_whole_sweep(report):
    rows = [ln.split()[1:] for ln in report if ln.startswith("slices ")]
    assert len(rows) > 1500
    for k, asked, eff, first, last in (map(int, r) for r in rows):
        sl = SK.slices(k, asked)
        assert len(sl) == eff, (k, asked)
        assert (sl[0][1], sl[-1][1]) == (first, last), (k, asked)
        assert sum(ln for _, ln in sl) == k // 16
