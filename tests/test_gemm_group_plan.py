# The grouped-GEMM plan without a GPU: table validation, ordering and the
# block id -> (problem, tile) map of marlin_amd/csrc/gemm_group_plan.h,
# driven by a stand-alone program (tests/data/gemm_group_plan_check.cpp)
# built under AddressSanitizer + UBSan with the runtimes linked statically
# into the program, so that it needs nothing from its environment. Where
# the toolchain cannot link the sanitizers the same program is built
# plain: its own checks still run.
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "gemm_group_plan_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


def test_gemm_group_plan_under_asan(tmp_path):
    exe = str(tmp_path / "group_plan_check")
    r = _build(exe, ["-fsanitize=address,undefined", "-static-libasan",
                     "-static-libubsan",
                     "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _build(exe, [])
    assert r.returncode == 0, r.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    m = re.search(r"gemm_group_plan OK (\d+) tables (\d+) checks", run.stdout)
    assert m, run.stdout[-2000:]
    # 10 fixed tables x 16 (type, op form, remap) + 40 generated
    assert int(m.group(1)) == 200


def test_problem_struct_matches_the_c_header():
    """The ctypes mirror of mx_gemm_problem_t: 12 eight-byte fields in the
    header's order."""
    import ctypes
    from marlin_amd.engine import MxGemmProblem
    names = [f for f, _ in MxGemmProblem._fields_]
    assert names == ["m", "k", "n", "dA", "a_off", "lda", "dB", "b_off",
                     "ldb", "dC", "c_off", "ldc"]
    assert ctypes.sizeof(MxGemmProblem) == 96
    hdr = open(os.path.join(ROOT, "include", "marlin_gpu.h")).read()
    body = hdr[hdr.index("int64_t m, k, n;"):hdr.index("} mx_gemm_problem_t;")]
    order = re.findall(r"\b(m|k|n|dA|a_off|lda|dB|b_off|ldb|dC|c_off|ldc)\b"
                       r"(?=\s*[,;])", re.sub(r"/\*.*?\*/", "", body))
    assert order == names
