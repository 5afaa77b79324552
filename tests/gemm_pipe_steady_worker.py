# Child process of test_gpu_gemm_pipe_steady.py (not a test module): the
# MARLIN_GEMM_* knobs are latched on first use, so each knob set needs a
# fresh process. With the knobs in the environment:
#   python tests/gemm_pipe_steady_worker.py exact -
#       runs _pipe_steady_cases.exact_cases(), the three transposed
#       products and the grouped launch, and prints ONE JSON line
#       {"cases": [record ...], "ops": [record ...], "group": record}
#   python tests/gemm_pipe_steady_worker.py bits <outdir>
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
import _exact_op as XO  # noqa: E402
import _grouped_cases as GC  # noqa: E402
import _pipe_steady_cases as SC  # noqa: E402
from marlin_amd import Engine  # noqa: E402
from marlin_amd import engine as E  # noqa: E402
from oracle import gen_matrix  # noqa: E402


def run_group(eng):
    """GROUP_SHAPES in one grouped fp64 NN call, beta 0, _exact images."""
    dt = np.float64
    nan = _exact._nan(dt)
    bufs, rows, imgs = [], [], []
    try:
        for (m, n, k) in SC.GROUP_SHAPES:
            c = _exact.Case(0, 0, m, n, k)
            a, b, c0, ref = _exact.gemm_inputs(c)
            lda, ldb = m + _exact.PAD, k + _exact.PAD
            cimg, sentinel = XO._c_image(c, c0, dt)
            dA = _exact._dev(eng, _exact._padded(a, lda, 0, nan), bufs)
            dB = _exact._dev(eng, _exact._padded(b, ldb, 0, nan), bufs)
            dC = _exact._dev(eng, cimg, bufs)
            rows.append(GC.row(m, k, n, dA, 0, lda, dB, 0, ldb, dC, 0,
                               cimg.shape[0]))
            imgs.append((m, n, dC, cimg, ref, sentinel))
        rc = eng.gemm_grouped_raw(rows, False, False, check=False)
        if rc != 0:
            return GC.fail(rc)
        out = {"rc": 0, "problems": [], "group": list(eng.last_gemm_group()),
               "loop": eng.last_gemm_loop()}
        for (m, n, dC, cimg, ref, sentinel) in imgs:
            got = np.empty_like(cimg)
            eng.download(got, dC, got.nbytes)
            out["problems"].append(_exact._check_image(
                got, m, n, ref, sentinel.view(_exact.UINT[dt])))
        return out
    finally:
        for d in bufs:
            eng.free(d)


def run_exact(eng):
    out = {"cases": [], "ops": [], "group": None}
    for c in SC.exact_cases():
        res = _exact.run_gemm_case(eng, c)
        res["id"] = _exact.case_id(c)
        res["loop"] = eng.last_gemm_loop() if res["rc"] == 0 else None
        out["cases"].append(res)
        if res["rc"] == -2:
            return out
    for form, c in SC.OP_CASES:
        res = XO.run_op_case(eng, c, *XO.FORMS[form])
        res["id"] = SC.op_id(form, c)
        out["ops"].append(res)
        if res["rc"] == -2:
            return out
    out["group"] = run_group(eng)
    return out


def run_bits(eng, outdir):
    sa, sb, sc = SC.PC.BITS_SEEDS
    out = []
    for fp32, beta, (m, n, k) in SC.BITS_CASES:
        dt = _exact.dtype_of(fp32)
        imgs = [np.asfortranarray(gen_matrix(r, c, s, dtype=dt))
                for (r, c, s) in ((m, k, sa), (k, n, sb), (m, n, sc))]
        bufs = []
        try:
            dA, dB, dC = (_exact._dev(eng, x, bufs) for x in imgs)
            rc = E.lib().mx_gemm_device_ex(eng._ctx, fp32, beta, m, k, n,
                                           dA, m, dB, k, dC, m)
            rec = {"id": SC.bits_id(fp32, beta, (m, n, k)), "rc": rc,
                   "loop": None}
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
        res = run_exact(eng) if mode == "exact" else run_bits(eng, arg)
    finally:
        eng.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
