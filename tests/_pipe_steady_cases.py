# Case tables of test_gpu_gemm_pipe_steady.py (shared with its child
# process gemm_pipe_steady_worker.py).
#
# The pipelined k-loop peels its last two steps; everything before them is
# the steady-state body. The existing tables run 1, 2, 3, 4, 5, 65 and 256
# tiles (and 32 for fp32). These add 6, 7, 8 and 9 tiles (K = 96 .. 144 at
# BK = 16): the steady-state body executed 4 .. 7 times, an even and an odd
# count twice each, so a body unrolled by two steps runs 2 or 3 times with
# and without a left-over step, and every buffer parity meets every exit.
# The exact-integer method and its bounds are tests/_exact.py's (K <= 512
# covers fp32).
import _exact
import _exact_op
import _pipelined_cases as PC
from _exact import Case

KS = (96, 112, 128, 144)
M = N = 256

RUNS = {
    "default": {},
    "pipe": {PC.LOOP_KNOB: "pipe"},
    "phase1": {"MARLIN_GEMM_PHASE": "1"},
    "phase8": {"MARLIN_GEMM_PHASE": "8"},
    "pipe-phase1": {PC.LOOP_KNOB: "pipe", "MARLIN_GEMM_PHASE": "1"},
    "pipe-phase8": {PC.LOOP_KNOB: "pipe", "MARLIN_GEMM_PHASE": "8"},
}


def loop_of(run):
    return "pipe" if run.startswith("pipe") else "default"


def exact_cases():
    return [Case(fp32, beta, M, N, k) for fp32 in (0, 1) for beta in (0, 1)
            for k in KS]


# one product per transposed form and one grouped launch, K = 112 (7 tiles)
OP_K = 112
OP_CASES = [("tn", Case(0, 0, 256, 384, OP_K)),
            ("nt", Case(0, 1, 384, 256, OP_K)),
            ("tt", Case(0, 0, 256, 384, OP_K))]
GROUP_SHAPES = [(256, 256, OP_K), (128, 384, OP_K)]      # (m, n, k), fp64


def op_id(form, c):
    return _exact_op.op_id(form, c)


# bit-identity with the two-barrier loop on non-integer data: 7 and 6
# tiles, 2 x 3 blocks
BITS_SHAPES = [(256, 384, 112), (256, 384, 96)]
BITS_LOOPS = ("twobar", "pipe", "default")


def bits_id(fp32, beta, shape):
    return f"{PC.bits_id(fp32, beta)}-{shape[0]}x{shape[1]}x{shape[2]}"


BITS_CASES = [(fp32, beta, s) for fp32, beta in PC.BITS_CASES
              for s in BITS_SHAPES]
