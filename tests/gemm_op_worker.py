# Child process of test_gpu_gemm_op.py (not a test module): the
# MARLIN_GEMM_* knobs are latched on first use, so each knob setting needs
# a fresh process. With the knobs in the environment,
#   python tests/gemm_op_worker.py
# runs the whole transposed-form exact table (_exact_op.table()) and
# prints ONE JSON line
#   {"cases": [{"id", "ok", "first_bad", "sentinel_inside", "pad_ok", "rc",
#               "cfg", "loop", "op"}, ...]}
# After a HIP failure (rc -2) nothing more is started on the device.
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _exact_op as XO  # noqa: E402
from marlin_amd import Engine  # noqa: E402


def main():
    eng = Engine(0)
    out = []
    try:
        for form, c in XO.table():
            res = XO.run_op_case(eng, c, *XO.FORMS[form])
            res["id"] = XO.op_id(form, c)
            out.append(res)
            if res["rc"] == -2:
                break
    finally:
        eng.close()
    print(json.dumps({"cases": out}), flush=True)


if __name__ == "__main__":
    main()
