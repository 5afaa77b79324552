# Child process of test_gpu_gemm_exact.py (not a test module): mxk_gemm
# latches MARLIN_GEMM_CFG / _REMAP / _BAND / _PHASE in function-local
# statics on first use, so every alternate config needs a fresh process.
# Run as `python tests/gemm_cfg_worker.py` with the knobs in the
# environment: opens Engine(0), runs the exact-integer case table for
# that environment and prints ONE JSON line
#   {"cases": [{"id", "ok", "first_bad", "sentinel_inside", "pad_ok",
#               "rc", "cfg"}, ...]}
# The parent asserts exactness and that each case ran the instantiation
# the environment was meant to select (cfg = mx_last_gemm_config).
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _exact  # noqa: E402
from marlin_amd import Engine  # noqa: E402


def main():
    eng = Engine(0)
    out = []
    try:
        for c in _exact.config_cases(os.environ):
            res = _exact.run_gemm_case(eng, c)
            res["id"] = _exact.case_id(c)
            out.append(res)
            if res["rc"] == -2:      # HIP failure: start nothing more
                break
    finally:
        eng.close()
    print(json.dumps({"cases": out}), flush=True)


if __name__ == "__main__":
    main()
