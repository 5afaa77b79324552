# The LDS staging layout of the GEMM kernels without a GPU: the DMA of one
# operand tile (marlin_amd/csrc/gemm_stage.h) replayed on the host for
# every (type, scheme, geometry) the kernels instantiate, by a stand-alone
# program built under AddressSanitizer and UBSan
# (tests/data/gemm_stage_check.cpp), with the sanitizer runtimes linked
# statically into the program so that it needs nothing from its
# environment. Where the toolchain cannot link the sanitizers the same
# program is built plain: its own checks still run.
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "gemm_stage_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


def test_gemm_stage_layout_under_asan(tmp_path):
    exe = str(tmp_path / "stage_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan",
                     "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    # 11 kernel geometries x 2 operands
    assert "gemm_stage OK 22" in run.stdout
