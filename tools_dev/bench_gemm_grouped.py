# Grouped GEMM against the per-product loop it replaces (diagnostics only).
#
#   python tools_dev/bench_gemm_grouped.py [--reps 5] [--out F]
#       [--arms trail,big,inverse,blockmul] [--inv-n 12000] [--mul-n 8000]
#
# One process, operands device-resident, the arms of every comparison
# alternated measurement by measurement so both see the same device state;
# one warm-up per arm (rep -1), then --reps repetitions. The comparison arm
# is always code that is not the grouped path: mx_gemm_device_op problem by
# problem, grouped=False in linalg, BlockMatrix._multiply_tile_chain.
#   trail     11 x 11 fp64 accumulate products 1024^3 sharing 11 A and 11 B
#             panels (one trailing update at base_size 1000): one grouped
#             call vs 121 plain calls. wall_ms is the host clock around the
#             synchronising entries, gemm_ms the hipEvent kernel time (summed
#             over the 121 launches for the loop), so launch + sync overhead
#             (wall - gemm) and under-filling (gemm) can be told apart.
#   big       8192^3 fp64 as a group of one vs mx_gemm_device_op (gemm_ms).
#   inverse   DenseVecMatrix.inverse(mode="dist", base_size=1000) at
#             --inv-n, grouped=False vs True (wall).
#   blockmul  BlockMatrix.multiply at --mul-n^2 in 8 x 8 blocks vs the kept
#             tile_dgemm_acc chain (wall).
# Every measurement is one JSON line in run order (appended to --out), then
# medians and spreads. Run the GPU step under its own time limit, e.g.
#   timeout -k 10 900 python tools_dev/bench_gemm_grouped.py --out F
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from marlin_amd import Engine, DenseVecMatrix  # noqa: E402
from marlin_amd import engine as E  # noqa: E402


def trail_arms(eng, nb=11, b=1024):
    def buf(seed):
        d = eng.alloc(b * b * 8)
        eng.fill_random(d, b * b, seed)
        return d
    A = [buf(100 + i) for i in range(nb)]
    B = [buf(200 + j) for j in range(nb)]
    C = [[buf(300 + i * nb + j) for j in range(nb)] for i in range(nb)]
    rows = [(b, b, b, A[i], 0, b, B[j], 0, b, C[i][j], 0, b)
            for i in range(nb) for j in range(nb)]
    flops = 2.0 * b ** 3 * nb * nb

    def out(wall, gemm, launches):
        return {"ms": wall, "gemm_ms": gemm, "launches": launches,
                "tflops_wall": flops / wall / 1e9,
                "tflops_gemm": flops / gemm / 1e9}

    def loop():
        gemm = 0.0
        t0 = time.perf_counter()
        for (m, k, n, a, _, lda, bb, _, ldb, c, _, ldc) in rows:
            rc = E.lib().mx_gemm_device_op(eng._ctx, 0, 1, 0, 0, m, k, n, a,
                                           lda, bb, ldb, c, ldc)
            assert rc == 0, rc
            gemm += eng.stats()["gemm_ms"]
        return out((time.perf_counter() - t0) * 1e3, gemm, len(rows))

    def grouped():
        t0 = time.perf_counter()
        eng.gemm_grouped_raw(rows, accumulate=True)
        wall = (time.perf_counter() - t0) * 1e3
        st = eng.stats()
        return out(wall, st["gemm_ms"], st["gemm_launches"])

    def free():
        for d in A + B + [c for r in C for c in r]:
            eng.free(d)
    return [("loop-121-plain", loop), ("grouped-1-launch", grouped)], free


def big_arms(eng, n=8192):
    bufs = [eng.alloc(n * n * 8) for _ in range(3)]
    eng.fill_random(bufs[0], n * n, 1)
    eng.fill_random(bufs[1], n * n, 2)
    a, b, c = bufs

    def res():
        ms = eng.stats()["gemm_ms"]
        return {"ms": ms, "tflops": 2.0 * n ** 3 / ms / 1e9}

    def plain():
        rc = E.lib().mx_gemm_device_op(eng._ctx, 0, 0, 0, 0, n, n, n, a, n, b,
                                       n, c, n)
        assert rc == 0, rc
        return res()

    def grouped():
        eng.gemm_grouped_raw([(n, n, n, a, 0, n, b, 0, n, c, 0, n)])
        return res()
    return ([("plain", plain), ("group-of-one", grouped)],
            lambda: [eng.free(d) for d in bufs])


def inverse_arms(eng, n):
    rng = np.random.default_rng(12)
    a = rng.random((n, n)) + n * np.eye(n)
    dvm = DenseVecMatrix(a, engine=eng)

    def run(g):
        t0 = time.perf_counter()
        dvm.inverse(mode="dist", base_size=1000, grouped=g)
        return {"ms": (time.perf_counter() - t0) * 1e3}
    return ([("grouped=False", lambda: run(False)),
             ("grouped=True", lambda: run(True))], lambda: None)


def blockmul_arms(eng, n):
    rng = np.random.default_rng(13)
    A = DenseVecMatrix(rng.random((n, n)), engine=eng).toBlockMatrix(8, 8)
    B = DenseVecMatrix(rng.random((n, n)), engine=eng).toBlockMatrix(8, 8)

    def run(f):
        t0 = time.perf_counter()
        f(B)
        ms = (time.perf_counter() - t0) * 1e3
        return {"ms": ms, "tflops": 2.0 * n ** 3 / ms / 1e9}
    return ([("tile-chain", lambda: run(A._multiply_tile_chain)),
             ("grouped", lambda: run(A.multiply))], lambda: None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--arms", default="trail,big,inverse,blockmul")
    ap.add_argument("--inv-n", type=int, default=12000)
    ap.add_argument("--mul-n", type=int, default=8000)
    ap.add_argument("--out")
    a = ap.parse_args()
    outf = open(a.out, "a") if a.out else None
    rows = []

    def emit(line):
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()

    eng = Engine(0)
    try:
        for key, make, reps in (
                ("trail", lambda: trail_arms(eng), a.reps),
                ("big", lambda: big_arms(eng), a.reps),
                ("inverse", lambda: inverse_arms(eng, a.inv_n), a.e2e_reps),
                ("blockmul", lambda: blockmul_arms(eng, a.mul_n), a.e2e_reps)):
            if key not in a.arms.split(","):
                continue
            arms, free = make()
            try:
                for rep in range(-1, reps):        # rep -1 is the warm-up
                    for label, fn in arms:
                        rec = dict(group=key, arm=label, rep=rep, **fn())
                        rows.append(rec)
                        emit(json.dumps(rec))
            finally:
                free()
    finally:
        eng.close()
    emit("# medians (warm-up excluded): group arm field median min max "
         "(max-min)/median")
    seen = []
    for r in rows:
        if (r["group"], r["arm"]) not in seen:
            seen.append((r["group"], r["arm"]))
    for g, arm in seen:
        for field in ("ms", "gemm_ms"):
            v = [r[field] for r in rows if (r["group"], r["arm"]) == (g, arm)
                 and r["rep"] >= 0 and field in r]
            if v:
                med = statistics.median(v)
                emit(f"# {g} {arm} {field} {med:.3f} {min(v):.3f} "
                     f"{max(v):.3f} {(max(v) - min(v)) / med * 100:.2f}%")


if __name__ == "__main__":
    main()
