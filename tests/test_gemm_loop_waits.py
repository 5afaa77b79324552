# What the compiled steady-state k-loop of the pipelined GEMM waits for
# (tools_dev/gemm_loop_waits.py on the device assembly of kernels.hip).
# CPU only: hipcc cross-compiles; skipped where hipcc is absent.
#
# The source of the pipelined loop reads quad q+1's fragments, then runs
# quad q's MFMAs; left to itself the machine scheduler moved reads of two
# quads into one and issued the last of them directly in front of an
# `s_waitcnt lgkmcnt(0)`, so every wave sat out an LDS round trip with no
# MFMA of its own queued, twice per k-step (profiles/r05_loop_waits.md).
# The loop now pins the reads behind the first MFMAs of the quad before.
# The rule is stated on the compiled code:
#   - no lgkmcnt wait of the steady-state body forces a ds_read issued
#     fewer than MIN_DIST MFMAs earlier (4 x 64 cycles: comfortably more
#     than an LDS round trip);
#   - the loop-top wait (the first behind the barrier, on the next tile's
#     quad-0 fragments) keeps the distance it had before the pinning;
#   - per k-step 64 MFMAs, one barrier and the geometry's DMA pieces (the
#     body holds two steps where it is unrolled for a constant buffer);
#   - no scratch, 2 waves per SIMD for fp64 and 4 for fp32.
import os
import shutil
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools_dev"))

import gemm_loop_waits as W  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None,
                                reason="hipcc not installed")

MIN_DIST = 4
# loop-top distance of the fp64 BK=16 forms before the pinning, by
# (TA, TB): 16 MFMAs of the last quad less the quad-0 read instructions
# (b64 reads pair up into ds_read2 differently per staging scheme)
TOP_DIST = {("0", "0"): 11, ("0", "1"): 9, ("1", "0"): 12, ("1", "1"): 10}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    out = tmp_path_factory.mktemp("gemm_asm") / "kernels.s"
    return W.kernels(W.compile_listing(out=str(out)))


def _pipelined(kernels):
    return {k: r for k, r in kernels.items() if r["key"]["PIPE"] == "1"}


def _name(r):
    return "<" + ",".join(r["key"].values()) + ">"


def test_every_listed_instantiation_is_compiled(kernels):
    pk = _pipelined(kernels)
    have = {(r["key"]["T"], r["key"]["BETA"], r["key"]["BK"], r["key"]["BM"],
             r["key"]["TA"], r["key"]["TB"], r["key"]["GRP"])
            for r in pk.values()}
    for t in ("double", "float"):
        for beta in "01":
            for grp in "01":
                for ta in "01":
                    for tb in "01":
                        assert (t, beta, "16", "128", ta, tb, grp) in have
            assert (t, beta, "32", "128", "0", "0", "0") in have
    for beta in "01":
        assert ("double", beta, "16", "256", "0", "0", "0") in have


def test_distance_rule(kernels):
    bad = []
    for r in _pipelined(kernels).values():
        forcing = [(n, d, top) for n, d, top in r["waits"] if d is not None]
        assert forcing, _name(r)
        for n, d, top in forcing:
            if d < MIN_DIST:
                bad.append(f"{_name(r)}: lgkmcnt({n}) forces a read "
                           f"{d} MFMAs old")
    assert not bad, "\n".join(bad)


def test_loop_top_wait_keeps_its_distance(kernels):
    for r in _pipelined(kernels).values():
        k = r["key"]
        if k["T"] != "double" or k["BK"] != "16":
            continue
        tops = [d for _, d, top in r["waits"] if top]
        steps = r["counts"]["mfma"] // 64
        assert len(tops) == steps, f"{_name(r)}: {W.waits_text(r['waits'])}"
        want = TOP_DIST[(k["TA"], k["TB"])]
        assert min(tops) >= want, \
            f"{_name(r)}: loop-top distance {tops}, was {want}"


def test_step_counts(kernels):
    for r in _pipelined(kernels).values():
        k, c = r["key"], r["counts"]
        steps = c["mfma"] // 64
        assert steps in (1, 2) and c["mfma"] == 64 * steps, _name(r)
        assert c["barrier"] == steps, _name(r)
        # 16-byte pieces, 64 lanes: tile bytes / 1 KiB, shared by the waves
        elem = 8 if k["T"] == "double" else 4
        pieces = ((int(k["BM"]) + 128) * int(k["BK"]) * elem
                  // (1024 * int(k["WM"]) * int(k["WN"])))
        assert c["dma"] == pieces * steps, _name(r)


def test_no_scratch_and_occupancy(kernels):
    for r in kernels.values():          # both loops
        assert r["scratch"] == 0, _name(r)
        assert r["occ"] == (2 if r["key"]["T"] == "double" else 4), _name(r)
