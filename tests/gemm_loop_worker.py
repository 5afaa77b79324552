# Child process of test_gpu_gemm_pipelined.py (not a test module): the
# MARLIN_GEMM_* knobs, MARLIN_GEMM_LOOP among them, are latched on first
# use, so each (variant, loop) pair needs a fresh process. With the knobs
# in the environment:
#   python tests/gemm_loop_worker.py exact <variant>
#       runs _pipelined_cases.exact_cases(variant) and prints ONE JSON line
#       {"cases": [{"id", "ok", "first_bad", "sentinel_inside", "pad_ok",
#                   "rc", "cfg", "loop"}, ...]}
#   python tests/gemm_loop_worker.py bits <outdir>
#       runs the non-integer cases, writes each downloaded C image to
#       <outdir>/<id>.npy and prints {"bits": [{"id", "rc", "loop"}, ...]}
# After a HIP failure (rc -2) nothing more is started on the device.
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _exact  # noqa: E402
import _pipelined_cases as PC  # noqa: E402
from marlin_amd import Engine  # noqa: E402
from marlin_amd import engine as E  # noqa: E402
from oracle import gen_matrix  # noqa: E402


def run_exact(eng, variant):
    out = []
    for c in PC.exact_cases(variant):
        res = _exact.run_gemm_case(eng, c)
        res["id"] = _exact.case_id(c)
        res["loop"] = eng.last_gemm_loop() if res["rc"] == 0 else None
        out.append(res)
        if res["rc"] == -2:
            break
    return {"cases": out}


def run_bits(eng, outdir):
    m, n, k = PC.BITS_SHAPE
    sa, sb, sc = PC.BITS_SEEDS
    out = []
    for fp32, beta in PC.BITS_CASES:
        dt = _exact.dtype_of(fp32)
        imgs = [np.asfortranarray(gen_matrix(r, c, s, dtype=dt))
                for (r, c, s) in ((m, k, sa), (k, n, sb), (m, n, sc))]
        bufs = []
        try:
            dA, dB, dC = (_exact._dev(eng, x, bufs) for x in imgs)
            rc = E.lib().mx_gemm_device_ex(eng._ctx, fp32, beta, m, k, n,
                                           dA, m, dB, k, dC, m)
            rec = {"id": PC.bits_id(fp32, beta), "rc": rc, "loop": None}
            if rc == 0:
                got = np.empty_like(imgs[2])
                eng.download(got, dC, got.nbytes)
                np.save(os.path.join(outdir, rec["id"] + ".npy"), got)
                rec["loop"] = eng.last_gemm_loop()
            out.append(rec)
            if rc == -2:
                break
        finally:
            for d in bufs:
                eng.free(d)
    return {"bits": out}


def main():
    mode, arg = sys.argv[1], sys.argv[2]
    eng = Engine(0)
    try:
        res = run_exact(eng, arg) if mode == "exact" else run_bits(eng, arg)
    finally:
        eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
