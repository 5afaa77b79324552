# Child process of test_gpu_gemm_rounding.py (not a test module): the
# MARLIN_GEMM_* knobs are latched on first use, so each variant of
# _rounding_cases.VARIANTS needs a fresh process. With the variant's knobs
# in the environment:
#   python tests/gemm_rounding_worker.py <variant> <outdir>
# runs _rounding_cases.variant_cases(variant) through mx_gemm_device_op (NN),
# writes each downloaded C interior to <outdir>/<id>.npy and prints ONE JSON
# line
#   {"cases": [{"id", "rc", "pad_ok", "sentinel_inside", "cfg", "loop"}, ...]}
# The parent measures the results against the high-precision reference and
# asserts that the variant really ran. After a HIP failure (rc -2) nothing
# more is started on the device.
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _rounding_cases as RC  # noqa: E402
from marlin_amd import Engine  # noqa: E402


def main():
    variant, outdir = sys.argv[1], sys.argv[2]
    eng = Engine(0)
    out = []
    try:
        for case in RC.variant_cases(variant):
            a, b, c0 = RC.case_inputs(case)
            res = RC.run_op(eng, case[0], "nn", a, b, c0)
            res["id"] = RC.variant_case_id(case)
            got = res.pop("got")
            if res["rc"] == 0:
                np.save(os.path.join(outdir, res["id"] + ".npy"), got)
            out.append(res)
            if res["rc"] == -2:
                break
    finally:
        eng.close()
    print(json.dumps({"cases": out}), flush=True)


if __name__ == "__main__":
    main()
