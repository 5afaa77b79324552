# The device triangular solve against what the decomposition tier did
# before it (diagnostics only; the numbers of profiles/trsm.md).
#
#   python tools_dev/bench_trsm.py [--mode entry|cholesky|solve|all]
#       [--reps 5] [--out F] [--n 1024] [--r 11264] [--chol-n 12000]
#       [--solve-n 8000] [--base 1000] [--fp32]
#
# One process; the two arms of a comparison alternate run by run so both
# see the same device state; one warm-up per arm, then --reps repetitions.
# wall_ms is the host clock around calls that end in a device synchronise,
# dev_ms the entry's own hipEvent time (mx_stats gemm_ms). One JSON line
# per compared point, the lists in run order with the warm-up first.
#   entry     mx_trsm_device, fp64 (fp32 with --fp32), n x r,
#             left-lower-unit and right-upper, operands resident. The other arm is the panel scale as
#             lu_decompose does it for the same panel: inverse of the
#             n x n block on the host, upload of the factor (and, on the
#             left, of its negation: the U12 panel and the -L^-1 A12 panel
#             are both formed), then the grouped GEMM over the panel's
#             n x n blocks. Its host_ms and upload_ms are reported apart.
#   cholesky  cholesky_decompose(mode="dist") at --chol-n, panel="trsm"
#             against panel="inverse", host input to host result.
#   solve     DenseVecMatrix.solve (its factorisation and its two device
#             substitutions timed apart) against inverse().multiply(b),
#             one right-hand side, at --solve-n.
# Run the GPU step under its own time limit, e.g.
#   timeout -k 10 900 python tools_dev/bench_trsm.py --out trsm_raw.jsonl
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


def bench_entry(eng, outf, n, r, reps, fp32=False):
    assert n % 128 == 0 and r % n == 0
    rng = np.random.RandomState(1)
    nblk = r // n
    for name, side, lower, unit in (("left-lower-unit", 0, 1, 1),
                                    ("right-upper", 1, 0, 0)):
        # well conditioned, so that solving in place again and again (the
        # timed loop does) keeps B finite
        t = rng.uniform(-1, 1, size=(n, n)) / n
        t = np.tril(t, -1) + np.eye(n) if lower else np.triu(t, 1) + 2 * np.eye(n)
        dT = eng.upload_matrix(t, fp32)
        shape = (r, n) if side else (n, r)
        dB = eng.upload_matrix(rng.uniform(-1, 1, size=shape), fp32)
        ldb = dB.pitch
        # the other arm's operands: the panel as nblk blocks of n x n
        blocks = [eng.upload_matrix(rng.uniform(-1, 1, size=(n, n)), fp32)
                  for _ in range(nblk)]
        rec = {"bench": "entry", "form": name, "n": n, "r": r,
               "fp64": not fp32,
               "trsm": {"wall_ms": [], "dev_ms": []},
               "inverse_gemm": {"wall_ms": [], "host_ms": [], "upload_ms": [],
                                "gemm_wall_ms": [], "dev_ms": []}}
        for _ in range(reps + 1):
            w, _ = timed(lambda: eng.trsm_raw(n, r, dT.buf, dT.pitch, dB.buf,
                                              ldb, side, lower, 0, unit,
                                              fp32))
            rec["trsm"]["wall_ms"].append(w)
            rec["trsm"]["dev_ms"].append(eng.stats()["gemm_ms"])

            def other():
                h, inv = timed(lambda: np.linalg.solve(t, np.eye(n)) if lower
                               else np.linalg.inv(t))
                if side:
                    u, ups = timed(lambda: [eng.upload_matrix(inv, fp32)])
                    probs = [(blk, ups[0], None) for blk in blocks]
                else:
                    u, ups = timed(lambda: [eng.upload_matrix(inv, fp32),
                                            eng.upload_matrix(-inv, fp32)])
                    probs = ([(ups[1], blk, None) for blk in blocks]
                             + [(ups[0], blk, None) for blk in blocks])
                g, done = timed(lambda: eng.gemm_grouped(probs))
                dev = eng.stats()["gemm_ms"]
                for d in ups + done:
                    d.free()
                return h, u, g, dev
            w, (h, u, g, dev) = timed(other)
            o = rec["inverse_gemm"]
            o["wall_ms"].append(w); o["host_ms"].append(h)
            o["upload_ms"].append(u); o["gemm_wall_ms"].append(g)
            o["dev_ms"].append(dev)
        assert np.isfinite(eng.download_matrix(dB)).all()
        rec["flops_trsm"] = float(n) * n * r
        rec["flops_inverse_gemm"] = 2.0 * n * n * n * (nblk if side
                                                       else 2 * nblk)
        emit(outf, rec)
        for d in [dT, dB] + blocks:
            d.free()


def spd(n, seed):
    rng = np.random.RandomState(seed)
    r = rng.uniform(0, 1, size=(n, n))
    return (r + r.T) / 2 + n * np.eye(n)


def bench_cholesky(eng, outf, n, base, reps):
    from marlin_amd import DenseVecMatrix
    a = spd(n, 2)
    dvm = DenseVecMatrix(a, engine=eng)
    rec = {"bench": "cholesky", "n": n, "base_size": base,
           "trsm": {"wall_ms": [], "rel_residual": None},
           "inverse": {"wall_ms": [], "rel_residual": None}}
    for it in range(reps + 1):
        for panel in ("trsm", "inverse"):
            w, blk = timed(lambda: dvm.choleskyDecompose(
                mode="dist", base_size=base, panel=panel))
            rec[panel]["wall_ms"].append(w)
            if it == 0:
                L = blk.toBreeze()
                rec[panel]["rel_residual"] = float(
                    np.max(np.abs(L @ L.T - a)) / np.max(np.abs(a)))
    emit(outf, rec)


def bench_solve(eng, outf, n, base, reps):
    from marlin_amd import DenseVecMatrix
    from marlin_amd.linalg import lu_decompose, lu_solve
    rng = np.random.RandomState(3)
    a = rng.uniform(0, 1, size=(n, n)) + n * np.eye(n)
    b = rng.uniform(-1, 1, size=n)
    dvm = DenseVecMatrix(a, engine=eng)
    rec = {"bench": "solve", "n": n, "base_size": base, "rhs": 1,
           "solve": {"wall_ms": [], "factor_ms": [], "lu_solve_ms": [],
                     "eta": None},
           "inverse_multiply": {"wall_ms": [], "eta": None}}

    def eta(x):
        res = a @ x - b
        return float(np.linalg.norm(res) / (np.linalg.norm(a)
                                            * np.linalg.norm(x)
                                            + np.linalg.norm(b)))
    for it in range(reps + 1):
        # solve() is these two calls; timed apart to show where it goes
        wf, (blocks, p_array) = timed(lambda: lu_decompose(dvm, "dist", base))
        ws, x = timed(lambda: lu_solve(blocks, p_array, b))
        rec["solve"]["wall_ms"].append(wf + ws)
        rec["solve"]["factor_ms"].append(wf)
        rec["solve"]["lu_solve_ms"].append(ws)
        w2, x2 = timed(lambda: dvm.inverse(mode="dist", base_size=base)
                       .multiply(b))
        rec["inverse_multiply"]["wall_ms"].append(w2)
        if it == 0:
            rec["solve"]["eta"] = eta(x)
            rec["inverse_multiply"]["eta"] = eta(np.asarray(x2))
            rec["numpy_eta"] = eta(np.linalg.solve(a, b))
    emit(outf, rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="all",
                    choices=["entry", "cholesky", "solve", "all"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--r", type=int, default=11264)
    ap.add_argument("--chol-n", type=int, default=12000)
    ap.add_argument("--solve-n", type=int, default=8000)
    ap.add_argument("--base", type=int, default=1000)
    ap.add_argument("--fp32", action="store_true",
                    help="the entry mode in fp32")
    args = ap.parse_args()
    from marlin_amd import Engine
    eng = Engine(0)
    outf = open(args.out, "a") if args.out else None
    try:
        if args.mode in ("entry", "all"):
            bench_entry(eng, outf, args.n, args.r, args.reps, args.fp32)
        if args.mode in ("cholesky", "all"):
            bench_cholesky(eng, outf, args.chol_n, args.base,
                           min(args.reps, 3))
        if args.mode in ("solve", "all"):
            bench_solve(eng, outf, args.solve_n, args.base,
                        min(args.reps, 3))
    finally:
        eng.close()
        if outf:
            outf.close()


if __name__ == "__main__":
    main()
