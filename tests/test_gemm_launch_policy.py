# The GEMM launch policy without a GPU: knob decoding, variant selection and
# the closed list of instantiations of marlin_amd/csrc/gemm_launch_policy.h,
# driven by a stand-alone program (tests/data/gemm_launch_policy_check.cpp)
# built under AddressSanitizer + UBSan with the runtimes linked statically
# into the program, so that it needs nothing from its environment. Where
# the toolchain cannot link the sanitizers the same program is built
# plain: its own checks still run.
#
# The GPU tests assert which variant ran against Python restatements of the
# policy (_exact.expected_config, _exact_op.expected_config,
# _pipelined_cases.expected_loop), one fresh process per knob set. Here the
# same restatements are compared with the C++ itself, for every knob set
# and case those tests use, so a disagreement shows before a GPU is needed.
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

import _exact
import _exact_op as XO
import _grouped_cases as GC
import _pipelined_cases as PC
from test_gpu_gemm_exact import CONFIGS as EXACT_CONFIGS
from test_gpu_gemm_op import CHILDREN as OP_CHILDREN

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "data", "gemm_launch_policy_check.cpp")
INC = os.path.join(ROOT, "marlin_amd", "csrc")


def _build(exe, flags):
    return subprocess.run(["g++", "-O1", "-g", "-std=c++17", *flags, SRC,
                           "-I", INC, "-o", exe],
                          capture_output=True, text=True)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("launch_policy") / "policy_check")
    r = _build(path, ["-fsanitize=address,undefined", "-static-libasan",
                      "-static-libubsan", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        r = _build(path, [])
    assert r.returncode == 0, r.stderr[-2000:]
    return path


def _run(exe, *args):
    run = subprocess.run([exe, *args], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout


def test_launch_policy_under_asan(exe):
    out = _run(exe)
    m = re.search(r"gemm_launch_policy OK (\d+) points (\d+) checks", out)
    assert m, out[-2000:]
    # 9 knob sets x 16 (type, beta, form) x (36 plain + 2 grouped) + 5
    # epilogue widths
    assert int(m.group(1)) == 9 * 16 * 38 + 5


# ---------------------------------------------------------------------------
# the knob sets of the GPU tests
def _knob_sets():
    sets = [dict(v, **l) for v in PC.VARIANTS.values()
            for l in PC.LOOPS.values()]
    sets += EXACT_CONFIGS + list(OP_CHILDREN.values()) + list(GC.LOOPS.values())
    out = []
    for s in sets:
        if s not in out:
            out.append(s)
    return out


def _knobs_id(knobs):
    return "+".join(f"{k[len('MARLIN_GEMM_'):]}={v}"
                    for k, v in knobs.items()) or "default"


def _loop_name(knobs):
    return knobs.get(PC.LOOP_KNOB, "default")


def _plain_cases(knobs):
    cases = _exact.config_cases(knobs)
    for variant in PC.VARIANTS:
        cases += [c for c in PC.exact_cases(variant) if c not in cases]
    return cases


def _select(exe, knobs, args):
    out = _run(exe, "--select", *(f"{k}={v}" for k, v in knobs.items()),
               *args)
    recs = [json.loads(ln) for ln in out.splitlines()]
    assert len(recs) == len(args)
    return recs


def _cfg(rec):
    return {k: rec[k] for k in ("is_fp32", "beta_one", "bk", "bm", "waves",
                                "band", "phase_mask")}


@pytest.mark.parametrize("knobs", _knob_sets(), ids=_knobs_id)
def test_python_restatements_match_the_policy(exe, knobs):
    loop = _loop_name(knobs)
    # plain entry
    cases = _plain_cases(knobs)
    recs = _select(exe, knobs, [f"{c.fp32},{c.beta},0,0,{c.M},{c.N},{c.K}"
                                for c in cases])
    for c, rec in zip(cases, recs):
        what = f"{_knobs_id(knobs)} {_exact.case_id(c)}"
        want = _exact.expected_config(knobs, c)
        assert _cfg(rec) == want, what
        assert rec["loop"] == PC.expected_loop(loop, want), what
        assert (rec["op"], rec["grouped"]) == ([0, 0], 0), what
    # transposed forms
    table = XO.table()
    recs = _select(exe, knobs, [
        f"{c.fp32},{c.beta},{XO.FORMS[f][0]},{XO.FORMS[f][1]},"
        f"{c.M},{c.N},{c.K}" for f, c in table])
    for (form, c), rec in zip(table, recs):
        what = f"{_knobs_id(knobs)} {XO.op_id(form, c)}"
        ta, tb = XO.FORMS[form]
        want = XO.expected_config(knobs, c, ta, tb)
        assert _cfg(rec) == want, what
        assert rec["loop"] == PC.expected_loop(loop, want), what
        assert (rec["op"], rec["grouped"]) == ([ta, tb], 0), what
    # grouped launch of _grouped_cases.SHAPES: the first table entry is the
    # one with the largest k (384 x 256 x 80: nbn = 2)
    m, n, k = max(GC.SHAPES, key=lambda s: s[2])
    recs = _select(exe, knobs, [
        f"g:{fp32},{beta},{GC.FORMS[form][0]},{GC.FORMS[form][1]},{n // 128}"
        for fp32, beta, form in GC.COMBOS])
    for (fp32, beta, form), rec in zip(GC.COMBOS, recs):
        what = f"{_knobs_id(knobs)} grouped {GC.combo_id(fp32, beta, form)}"
        want = _exact.expected_config(knobs, _exact.Case(fp32, beta, m, n, k))
        want.update(bk=16, bm=128, waves=4, phase_mask=0)
        assert _cfg(rec) == want, what
        assert rec["loop"] == PC.expected_loop(loop, want), what
        assert (rec["op"], rec["grouped"]) == (list(GC.FORMS[form]), 1), what


def test_grouped_expectations_of_the_gpu_test(exe):
    """What test_gpu_gemm_grouped.py asserts, literally: band 2, and under a
    forced loop that loop; with no knob fp64 pipelined, fp32 two-barrier."""
    for loop, knobs in dict(GC.LOOPS, default={}).items():
        recs = _select(exe, knobs, [
            f"g:{fp32},{beta},{GC.FORMS[form][0]},{GC.FORMS[form][1]},2"
            for fp32, beta, form in GC.COMBOS])
        for (fp32, beta, form), rec in zip(GC.COMBOS, recs):
            assert _cfg(rec) == {"is_fp32": fp32, "beta_one": beta, "bk": 16,
                                 "bm": 128, "waves": 4, "band": 2,
                                 "phase_mask": 0}
            want = {"pipe": 1, "twobar": 0, "default": 0 if fp32 else 1}[loop]
            assert rec["loop"] == want


# ---------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_compiled_kernels_are_exactly_the_list(exe, tmp_path):
    """The gemm_mfma_kernel instantiations in the device code of kernels.hip
    are the members of the policy's list, no more and no fewer."""
    sys.path.insert(0, os.path.join(ROOT, "tools_dev"))
    import gemm_loop_waits as W
    listed = [tuple(ln.split(",")) for ln in _run(exe, "--list").splitlines()]
    assert len(listed) == len(set(listed)) == 77
    compiled = set(W.kernels(W.compile_listing(out=str(tmp_path / "k.s"))))
    assert compiled - set(listed) == set(), "compiled but not listed"
    assert set(listed) - compiled == set(), "listed but not compiled"
