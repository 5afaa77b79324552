# Case tables of test_gpu_gemm_pipelined.py (shared with its child
# process gemm_loop_worker.py and the CPU-only test_pipelined_cases.py).
#
# The exact-integer method is tests/_exact.py's; these tables add what the
# pipelined k-loop needs on top of the existing ntiles 1, 2, 3, 5:
#   - 4 tiles (K = 64): the first even count above 2, where the peeled
#     last two steps follow exactly two steady-state steps;
#   - the longest K _exact proves exact (4096 fp64 = 256 tiles, 512 fp32
#     = 32 tiles): the steady state, both buffers reused many times;
#   - the same long K under every knob that changes the loop's geometry
#     or its tile order (bk32, bm256, MARLIN_GEMM_PHASE), at M = 384
#     (bm256 must fall back) and M = 512 (bm256 really runs).
# Every table is run under the per-variant default and under both forced
# loops (MARLIN_GEMM_LOOP=twobar / =pipe): fp32 at BK=16 keeps the
# two-barrier loop by default, so only "pipe" reaches its pipelined code.
import _exact
from _exact import Case

LOOP_KNOB = "MARLIN_GEMM_LOOP"
LOOPS = {"default": {}, "twobar": {LOOP_KNOB: "twobar"},
         "pipe": {LOOP_KNOB: "pipe"}}

VARIANTS = {
    "base": {},
    "bk32": {"MARLIN_GEMM_CFG": "bk32"},
    "bm256": {"MARLIN_GEMM_CFG": "bm256"},
    "phase1": {"MARLIN_GEMM_PHASE": "1"},
    "phase8": {"MARLIN_GEMM_PHASE": "8"},
}

KNOBS = ("MARLIN_GEMM_CFG", "MARLIN_GEMM_REMAP", "MARLIN_GEMM_BAND",
         "MARLIN_GEMM_PHASE", LOOP_KNOB)


def long_k(fp32):
    return _exact.F32_KMAX if fp32 else _exact.F64_KMAX


def exact_cases(variant):
    shapes = ([(256, 256, 64), (256, 256, None)] if variant == "base"
              else [(384, 256, None), (512, 256, None)])
    out = []
    for fp32 in (0, 1):
        for beta in (0, 1):
            for (m, n, k) in shapes:
                out.append(Case(fp32, beta, m, n, k or long_k(fp32)))
    return out


def expected_loop(loop, cfg):
    """What mx_last_gemm_loop must report (1 = pipelined, 0 = two-barrier)
    for a launch whose mx_last_gemm_config is cfg: restatement of the
    launcher's per-variant default, where only fp32 at BK=16 keeps the
    two-barrier loop."""
    if loop != "default":
        return 0 if loop == "twobar" else 1
    return 0 if (cfg["is_fp32"] and cfg["bk"] == 16) else 1


# Bit-identity of the two loops on non-integer data: 65 tiles (odd), more
# than one block in both directions.
BITS_SHAPE = (256, 384, 1040)
BITS_CASES = [(fp32, beta) for fp32 in (0, 1) for beta in (0, 1)]
BITS_SEEDS = (0x51A7E, 0xB17C0DE, 0xC0FFEE)     # A, B, C0


def bits_id(fp32, beta):
    return f"{'f32' if fp32 else 'f64'}-b{beta}"
