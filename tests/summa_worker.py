# Child process of test_gpu_summa_exact.py (not a test module): the
# SUMMA loop latches MARLIN_SUMMA_KB in a function-local static on first
# use, so a non-default panel width at the REAL entries needs a fresh
# process. Run as `python tests/summa_worker.py` with the knob in the
# environment: opens Engine(0), comm_init(0, 1), runs the real one-rank
# device and host entries of both types on _exact_summa.KNOB_SHAPE with
# exact data and prints ONE JSON line
#   {"runs": [{"id", "ok", "first_bad", "sentinel_inside", "pad_ok",
#              "pad_rows_zero", "pad_cols_zero", "rc", "launches",
#              "comm_ms"}, ...]}
# The parent asserts exactness, the pad contract and that gemm_launches
# is the panel count of the width the environment asked for.
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _exact_summa as S  # noqa: E402
from marlin_amd import Engine  # noqa: E402


def main():
    eng = Engine(0)
    out = []
    try:
        eng.comm_init(0, 1, Engine.comm_id())
        for fp32 in (0, 1):
            c = S.SummaCase(fp32, 1, 1, *S.KNOB_SHAPE, S.KNOB_KB)
            for where, run in (("device", S.run_real_device),
                               ("host", S.run_real_host)):
                res = run(eng, c, "summa")
                res["id"] = f"{'f32' if fp32 else 'f64'}-{where}"
                out.append(res)
                if res["rc"] == -2:      # HIP failure: start nothing more
                    break
            else:
                continue
            break
    finally:
        eng.close()
    print(json.dumps({"runs": out}), flush=True)


if __name__ == "__main__":
    main()
