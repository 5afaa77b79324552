# Child process of test_gpu_gemm_splitk.py (not a test module): the
# MARLIN_GEMM_LOOP knob is latched on first use, so each loop needs a fresh
# process. With the knob in the environment,
#   python tests/gemm_splitk_worker.py
# re-runs the fold cases of _splitk_cases.FOLD_CASES and prints ONE JSON
# line {"first": [S, bytes] before any call, "fold": {case id: record}}.
# After a HIP failure (rc -2) nothing more is started on the device.
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _splitk_cases as SK  # noqa: E402
from marlin_amd import Engine  # noqa: E402


def main():
    out = {"fold": {}}
    eng = Engine(0)
    try:
        out["first"] = list(eng.last_gemm_splitk())
        for case in SK.FOLD_CASES:
            res = SK.run_fold(eng, *case)
            out["fold"][SK.fold_id(*case)] = res
            if res["rc"] == -2:
                return out
    finally:
        eng.close()
        print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
