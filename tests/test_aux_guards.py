# The argument checks of the auxiliary entries without a GPU
# (marlin_amd/csrc/aux_guards.h: mx_fill_random, mx_zero_pad,
# mx_transpose_device, mx_dgemv_device, the pitched and whole-buffer
# transfers, mx_memset, mx_map), driven by a stand-alone program
# (tests/data/aux_guards_check.cpp) built under AddressSanitizer + UBSan
# with the runtimes linked statically into the program, so that it needs
# nothing from its environment. Where the toolchain cannot link the
# sanitizers the same program is built plain, with a warning in the test
# report: its own checks still run.
# The program sweeps each check over small values and over values near
# INT64_MAX, compares every decision with 128-bit arithmetic and replays
# the addressing of each accepted small call on a heap block of exactly
# the buffer's size; here a handful of its decisions are compared with the
# Python restatement of tests/_aux_cases.py, which the GPU tests use to
# pick their cases. This is where the guards are shown not to be vacuous:
# the refusals themselves are never provoked against an unguarded build.
import os
import subprocess
import warnings

import pytest

import _aux_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "aux_guards_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")

CHECKS = ["fill_random", "zero_pad", "transpose", "gemv", "copy2d", "bytes",
          "map_op"]


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aux") / "aux_guards_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        # not silently: the run below then proves less, and says so
        warnings.warn("aux_guards_check built WITHOUT sanitizers, the "
                      "sanitizer link failed: " + r.stderr[-300:])
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout.splitlines()


def test_aux_guards_under_asan(report):
    assert report[-1].startswith("aux_guards OK "), report[-5:]
    assert int(report[-1].split()[2]) > 10000


def test_every_check_accepts_and_refuses(report):
    rows = {ln.split()[1]: ln.split() for ln in report
            if ln.startswith("check ")}
    assert sorted(rows) == sorted(CHECKS)
    for name, r in rows.items():
        assert r[2] == "accepted" and r[4] == "refused", r
        assert int(r[3]) > 0 and int(r[5]) > 0, r


def _decisions(report, name):
    rows = [[int(v) for v in ln.split()[2:]] for ln in report
            if ln.startswith(f"decide {name} ")]
    assert rows, name
    seen = {r[-1] for r in rows}
    assert seen == {0, 1}, (name, seen)       # both sides of the edge
    return rows


def test_restatement_agrees_with_the_header(report):
    for fp32, nbytes, n, ok in _decisions(report, "fill"):
        assert AC.fill_ok(nbytes, fp32, n) == bool(ok), (fp32, nbytes, n)
    for fp32, nbytes, rt, ct, ld, m, n, ok in _decisions(report, "zero_pad"):
        assert AC.zero_pad_ok(nbytes, fp32, rt, ct, ld, m, n) == bool(ok), \
            (fp32, nbytes, rt, ct, ld, m, n)
    for fp32, bi, bo, m, n, ok in _decisions(report, "transpose"):
        assert AC.transpose_ok(fp32, m, n, bi, bo) == bool(ok), \
            (fp32, bi, bo, m, n)
    for nbytes, m, n, lda, ok in _decisions(report, "gemv"):
        assert AC.gemv_ok(nbytes, m, n, lda) == bool(ok), (nbytes, m, n, lda)
    for elem, nbytes, off, pitch, m, n, ok in _decisions(report, "copy2d"):
        assert AC.copy2d_ok(nbytes, elem, off, pitch, m, n) == bool(ok), \
            (elem, nbytes, off, pitch, m, n)
    for op, ok in _decisions(report, "map_op"):
        assert AC.map_op_ok(op) == bool(ok), op


def test_restatement_edges():
    # the least overstep of each rule, as the GPU refusal test uses them
    assert AC.fill_ok(800, 0, 100) and not AC.fill_ok(800, 0, 101)
    assert AC.fill_ok(800, 1, 200) and not AC.fill_ok(800, 1, 201)
    assert not AC.fill_ok(800, 0, -1)
    assert AC.zero_pad_ok(8 * 8 * 3, 0, 8, 3, 8, 8, 3)
    assert not AC.zero_pad_ok(8 * 8 * 3 - 8, 0, 8, 3, 8, 8, 3)
    assert not AC.zero_pad_ok(8 * 9 * 3, 0, 8, 3, 7, 8, 3)      # ld < rows
    assert not AC.zero_pad_ok(8 * 9 * 3, 0, 8, 3, 8, 9, 3)      # m > rows
    assert AC.gemv_ok(8 * (2 * 9 + 8), 8, 3, 9)
    assert not AC.gemv_ok(8 * (2 * 9 + 8) - 8, 8, 3, 9)
    assert not AC.gemv_ok(8 * 100, 8, 3, 7)                     # lda < m
    assert AC.copy2d_ok(200, 8, 8, 8, 8, 3)
    assert not AC.copy2d_ok(200, 8, 16, 8, 8, 3)
    assert not AC.transpose_ok(0, 3, 3, 72, 72, same=True)
    assert AC.bytes_ok(8, 0) and AC.bytes_ok(8, 8)
    assert not AC.bytes_ok(8, -1) and not AC.bytes_ok(8, 9)
    # values whose products leave 64 bits: Python ints simply carry on
    big = 2 ** 63 - 1
    assert not AC.fill_ok(big, 0, big)
    assert not AC.gemv_ok(big, big // 8, big, big)
    assert AC.gemv_ok(big, big // 8, 1, big)
