# Wall time and mx_stats of the host-buffer entries, which bench.py does not
# cover: Engine.dgemm at 4096^3 and at ragged 4000 x 4100 x 3900,
# sgemm_transpose_add at 4096^3 and map_op on 2^24 elements. The operands
# are pageable numpy arrays, so the PCIe copies dominate every wall time;
# what this measures is whether the staging sequence around them moved.
# One JSON line per arm: the wall time of each repetition (ms, host clock
# around the synchronising entry) and the stats of the last one.
#
#   python tools_dev/bench_host_entries.py [--reps 5] [--tag NAME]
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marlin_amd import Engine  # noqa: E402


def _rand(shape, dt, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal(shape).astype(dt))


def arms():
    d, f = np.float64, np.float32
    a, b = _rand((4096, 4096), d, 1), _rand((4096, 4096), d, 2)
    yield "dgemm_4096", lambda e: e.dgemm(a, b)
    ar, br = _rand((4000, 4100), d, 3), _rand((4100, 3900), d, 4)
    yield "dgemm_4000x4100x3900", lambda e: e.dgemm(ar, br)
    af, bf, cf = (_rand((4096, 4096), f, s) for s in (5, 6, 7))
    yield "sgemm_transpose_add_4096", lambda e: e.sgemm_transpose_add(
        af, bf, add_c=cf)
    x, y = _rand((1 << 24,), d, 8), _rand((1 << 24,), d, 9)
    yield "map_add_2^24", lambda e: e.map_op("add", x, y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    eng = Engine(0)
    try:
        for name, call in arms():
            call(eng)                       # warm-up: allocates the workspaces
            wall = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                call(eng)
                wall.append(round((time.perf_counter() - t0) * 1e3, 3))
            # mx_map keeps no stats: mx_stats would show the previous arm's
            st = None if name.startswith("map") else eng.stats()
            print(json.dumps({
                "tag": args.tag, "arm": name, "wall_ms": wall,
                "wall_ms_median": float(np.median(wall)),
                "stats": st and {k: round(float(st[k]), 4) for k in (
                    "h2d_ms", "gemm_ms", "total_ms", "gemm_launches")},
            }), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
