# Host side of mx_gemm_op without a GPU: the padding arithmetic, pitches
# and copy extents (marlin_amd/csrc/gemm_op_layout.h) replayed on heap
# buffers by a stand-alone program built under AddressSanitizer
# (tests/data/gemm_op_layout_check.cpp), with the sanitizer runtime linked
# statically into the program so that it needs nothing from its
# environment. Where the toolchain cannot link the sanitizer the same
# program is built plain: its own extent and value checks still run.
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "gemm_op_layout_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


def test_gemm_op_host_layout_under_asan(tmp_path):
    exe = str(tmp_path / "layout_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan",
                     "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "gemm_op_layout OK 28" in run.stdout
