# The device LU factorisation against what the decomposition tier did
# before it (diagnostics only; the numbers of profiles/getrf.md).
#
#   python tools_dev/bench_getrf.py [--mode entry|lu|solve|all] [--reps 3]
#       [--out F] [--entry-n 1024,4096,8000] [--n 8000] [--base 1000]
#       [--fp32]
#
# One process; the arms of a comparison alternate run by run so all see the
# same device state; one warm-up per arm, then --reps repetitions. wall_ms
# is the host clock around calls that end in a device synchronise, dev_ms
# the entry's own hipEvent time (mx_stats gemm_ms). One JSON line per
# compared point, the lists in run order with the warm-up first.
#   entry  mx_getrf_device, fp64 (fp32 with --fp32), on a freshly uploaded
#          resident image (the upload is outside the clock), at each
#          --entry-n.
#   lu     lu_decompose(mode="dist", base_size=--base) at --n, panel="device"
#          against panel="host", host matrix in, host factor out.
#   solve  DenseVecMatrix.solve at --n, one right-hand side: factor="device"
#          (lu_factor_device and DeviceLU.solve timed apart) against
#          factor="host" (lu_decompose and lu_solve timed apart) and against
#          inverse().multiply(b).
# Run the GPU step under its own time limit, e.g.
#   timeout -k 10 600 python tools_dev/bench_getrf.py --out getrf_raw.jsonl
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(outf, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if outf:
        outf.write(line + "\n")
        outf.flush()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def dominant(n, seed):
    rng = np.random.RandomState(seed)
    return np.asfortranarray(rng.uniform(0, 1, size=(n, n)) + n * np.eye(n))


def bench_entry(eng, outf, n, reps, fp32=False):
    a = dominant(n, 1)
    npad = (n + 127) // 128 * 128
    d_piv = eng.alloc(npad * 4)
    rec = {"bench": "entry", "n": n, "fp64": not fp32,
           "flops": 2.0 * n ** 3 / 3,
           "getrf": {"wall_ms": [], "dev_ms": [], "info": []}}
    try:
        for it in range(reps + 1):
            dA = eng.upload_matrix(a, fp32)
            try:
                w, (_, info) = timed(lambda: eng.getrf_raw(n, dA.buf, dA.pitch,
                                                           d_piv, fp32))
                rec["getrf"]["wall_ms"].append(w)
                rec["getrf"]["dev_ms"].append(eng.stats()["gemm_ms"])
                rec["getrf"]["info"].append(info)
                if it == 0:
                    lu = eng.download_matrix(dA)
                    piv = np.empty(npad, dtype=np.int32)
                    eng.download(piv, d_piv, piv.nbytes)
                    L = np.tril(lu, -1) + np.eye(n)
                    rec["rel_residual"] = float(
                        np.max(np.abs(a[piv[:n], :] - L @ np.triu(lu)))
                        / np.max(np.abs(a)))
            finally:
                dA.free()
    finally:
        eng.free(d_piv)
    emit(outf, rec)


def bench_lu(eng, outf, n, base, reps):
    from marlin_amd import DenseVecMatrix
    a = dominant(n, 2)
    dvm = DenseVecMatrix(a, engine=eng)
    rec = {"bench": "lu_decompose", "n": n, "base_size": base,
           "device": {"wall_ms": [], "rel_residual": None},
           "host": {"wall_ms": [], "rel_residual": None}}
    for it in range(reps + 1):
        for panel in ("device", "host"):
            w, (blk, p) = timed(lambda: dvm.luDecompose(
                mode="dist", base_size=base, panel=panel))
            rec[panel]["wall_ms"].append(w)
            if it == 0:
                lu = blk.toBreeze()
                L = np.tril(lu, -1) + np.eye(n)
                rec[panel]["rel_residual"] = float(
                    np.max(np.abs(a[p, :] - L @ np.triu(lu)))
                    / np.max(np.abs(a)))
    emit(outf, rec)


def bench_solve(eng, outf, n, base, reps):
    from marlin_amd import DenseVecMatrix
    from marlin_amd.linalg import lu_decompose, lu_factor_device, lu_solve
    rng = np.random.RandomState(3)
    a = rng.uniform(0, 1, size=(n, n)) + n * np.eye(n)
    b = rng.uniform(-1, 1, size=n)
    dvm = DenseVecMatrix(a, engine=eng)
    rec = {"bench": "solve", "n": n, "base_size": base, "rhs": 1,
           "device": {"wall_ms": [], "factor_ms": [], "solve_ms": [],
                      "eta": None},
           "host": {"wall_ms": [], "factor_ms": [], "lu_solve_ms": [],
                    "eta": None},
           "inverse_multiply": {"wall_ms": [], "eta": None}}

    def eta(x):
        res = a @ x - b
        return float(np.linalg.norm(res) / (np.linalg.norm(a)
                                            * np.linalg.norm(x)
                                            + np.linalg.norm(b)))
    for it in range(reps + 1):
        # solve(factor="device") is these calls; timed apart
        wf, f = timed(lambda: lu_factor_device(dvm))
        ws, xd = timed(lambda: f.solve(b))
        wr, _ = timed(f.free)
        rec["device"]["wall_ms"].append(wf + ws + wr)
        rec["device"]["factor_ms"].append(wf)
        rec["device"]["solve_ms"].append(ws)
        # solve(factor="host") likewise
        wf, (blocks, p_array) = timed(lambda: lu_decompose(dvm, "dist", base))
        ws, xh = timed(lambda: lu_solve(blocks, p_array, b))
        rec["host"]["wall_ms"].append(wf + ws)
        rec["host"]["factor_ms"].append(wf)
        rec["host"]["lu_solve_ms"].append(ws)
        w2, x2 = timed(lambda: dvm.inverse(mode="dist", base_size=base)
                       .multiply(b))
        rec["inverse_multiply"]["wall_ms"].append(w2)
        if it == 0:
            rec["device"]["eta"] = eta(xd)
            rec["host"]["eta"] = eta(xh)
            rec["inverse_multiply"]["eta"] = eta(np.asarray(x2))
            rec["numpy_eta"] = eta(np.linalg.solve(a, b))
    emit(outf, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all",
                    choices=["entry", "lu", "solve", "all"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--entry-n", default="1024,4096,8000")
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--base", type=int, default=1000)
    ap.add_argument("--fp32", action="store_true",
                    help="the entry mode in fp32")
    args = ap.parse_args()
    from marlin_amd import Engine
    eng = Engine(0)
    outf = open(args.out, "a") if args.out else None
    try:
        if args.mode in ("entry", "all"):
            for n in (int(v) for v in args.entry_n.split(",")):
                bench_entry(eng, outf, n, max(args.reps, 5), args.fp32)
        if args.mode in ("lu", "all"):
            bench_lu(eng, outf, args.n, args.base, args.reps)
        if args.mode in ("solve", "all"):
            bench_solve(eng, outf, args.n, args.base, args.reps)
    finally:
        eng.close()
        if outf:
            outf.close()


if __name__ == "__main__":
    main()
