# The staging of the host-buffer entries without a GPU: the images, their
# byte sizes and the stage-in / stage-out code of
# marlin_amd/csrc/host_stage.h, run with a heap backend by a stand-alone
# program built under AddressSanitizer + UBSan
# (tests/data/host_stage_check.cpp), with the sanitizer runtime linked
# statically into the program so that it needs nothing from its
# environment. Where the toolchain cannot link the sanitizer the same
# program is built plain: its own extent and value checks still run.
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "host_stage_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


def test_host_stage_under_asan(tmp_path):
    exe = str(tmp_path / "host_stage_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan",
                     "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    # the 28 multiply forms, then every other image and the size sweep
    assert "gemm_op_layout OK 28" in run.stdout
    assert "host_stage OK 616 images 3248 size checks" in run.stdout
