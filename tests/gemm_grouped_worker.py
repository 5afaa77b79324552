# Child process of test_gpu_gemm_grouped.py (not a test module): the
# MARLIN_GEMM_LOOP knob is latched on first use, so each loop needs a fresh
# process. With the knob in the environment,
#   python tests/gemm_grouped_worker.py
# runs every (type, beta, op form) of _grouped_cases.run_exact_group and
# the bit-identity runs, and prints ONE JSON line
#   {"exact": {combo id: record}, "bits": {"f64-b0": record, ...}}
# After a HIP failure (rc -2) nothing more is started on the device.
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _grouped_cases as GC  # noqa: E402
from marlin_amd import Engine  # noqa: E402


def main():
    out = {"exact": {}, "bits": {}}
    eng = Engine(0)
    try:
        for fp32, beta, form in GC.COMBOS:
            res = GC.run_exact_group(eng, fp32, beta, form)
            out["exact"][GC.combo_id(fp32, beta, form)] = res
            if res["rc"] == -2:
                return out
        for fp32 in (0, 1):
            for beta in (0, 1):
                res = GC.run_bits(eng, fp32, beta)
                out["bits"][GC.combo_id(fp32, beta, "nn")] = res
                if res["rc"] == -2:
                    return out
    finally:
        eng.close()
        print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    main()
