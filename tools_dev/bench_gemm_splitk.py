# Split-K GEMM against the unsplit launch (diagnostics only; the numbers of
# profiles/gemm_splitk.md).
#
#   python tools_dev/bench_gemm_splitk.py --mode sweep|report|reduce
#       [--reps 3] [--out F] [--kmax 1048576] [--operand-gib 16]
#   python tools_dev/bench_gemm_splitk.py --analyze F.jsonl
#   python tools_dev/bench_gemm_splitk.py --trace T.csv --label L [--out F]
#
# One process, operands device-resident (two big random buffers, every
# shape a prefix of them: the values do not matter here), the arms of a
# comparison alternated measurement by measurement so all see the same
# device state; one warm-up per arm, then --reps repetitions. The plain arm
# is always mx_gemm_device_op, never the split entry at S = 1. wall_ms is
# the host clock around the synchronising entry, gemm_ms its hipEvent time
# (for a split call: table copy + grouped GEMM + reduce).
#   sweep   fp64 / fp32 x TN / NN x tiles 1, 4, 16, 64, 256 x k = 512, 2048,
#           .. (x4 steps) and --kmax x explicit S = 1 (plain), 2, 4, .. up to
#           min(resident / tiles, k / 16): what fixes the policy constants.
#   report  the named shapes, plain against slices = 0 (auto).
#   reduce  split calls with a short k, each followed by mx_map add on host
#           arrays of the same byte count (S + 1) * m * n * elem. Neither
#           entry times its kernel alone: run this mode under a kernel
#           trace (rocprofv3 --kernel-trace -f csv -- python ...); --trace
#           then prints the two kernels' durations from that trace.
#   --analyze  per candidate (fill, MX_SPLITK_MIN_KSTEPS) the swept points
#           where the auto rule would pick an S that ran slower than plain.
# One JSON line per compared point (appended to --out): per arm the
# effective S and the wall_ms / gemm_ms lists in run order, the warm-up
# first; a sweep line keeps only wall_ms per S (S = 1 is the plain arm),
# without the warm-up. Run the GPU step under its own time limit, e.g.
#   timeout -k 10 900 python tools_dev/bench_gemm_splitk.py --mode sweep
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE_DIMS = {1: 128, 4: 256, 16: 512, 64: 1024, 256: 2048}
FORMS = {"nn": (0, 0), "tn": (1, 0)}


def resident(fp32, cus):
    return cus * (4 if fp32 else 2)


class Bench:
    def __init__(self, out):
        from marlin_amd import Engine
        from marlin_amd import engine as E
        self.E = E
        self.eng = Engine(0)
        self.cus = self.eng.device_info()[0]
        self.outf = open(out, "a") if out else None
        self.bufs = {}

    def emit(self, rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if self.outf:
            self.outf.write(line + "\n")
            self.outf.flush()

    def buf(self, name, nbytes, seed=None, fp32=0):
        """A cached device buffer of at least nbytes per (name, type),
        filled with U[0, 1) of that type when seeded."""
        name = f"{name}{fp32}"
        have = self.bufs.get(name)
        if have and have[1] >= nbytes:
            return have[0]
        if have:
            self.eng.free(have[0])
        d = self.eng.alloc(nbytes)
        if seed is not None:
            self.eng.fill_random(d, nbytes // (4 if fp32 else 8), seed,
                                 bool(fp32))
        self.bufs[name] = (d, nbytes)
        return d

    def close(self):
        for d, _ in self.bufs.values():
            self.eng.free(d)
        self.eng.close()

    def call(self, fp32, form, m, n, k, dA, dB, dC, s):
        """One timed call: s = None is the plain entry, else the split
        entry with slices = s. Returns (wall_ms, gemm_ms, effective S)."""
        ta, tb = FORMS[form]
        lda, ldb = (k if ta else m), (n if tb else k)
        t0 = time.perf_counter()
        if s is None:
            rc = self.E.lib().mx_gemm_device_op(
                self.eng._ctx, fp32, 0, ta, tb, m, k, n, dA, lda, dB, ldb,
                dC, m)
        else:
            rc = self.eng.gemm_splitk_raw(m, k, n, dA, lda, dB, ldb, dC, m, s,
                                          fp32, False, ta, tb, check=False)
        wall = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        eff = 1 if s is None else self.eng.last_gemm_splitk()[0]
        return wall, self.eng.stats()["gemm_ms"], eff

    def compare(self, group, fp32, form, m, n, k, arms, reps, same_ab=False):
        """arms: [(label, s)], alternated; the first round is the warm-up.
        The sweep keeps the wall clock only (what --analyze reads)."""
        elem = 4 if fp32 else 8
        dA = self.buf("A", m * k * elem, 0xA5, fp32)
        dB = dA if same_ab else self.buf("B", k * n * elem, 0xB5, fp32)
        dC = self.buf("C", m * n * elem, None, fp32)
        out = {label: dict(S=0, wall_ms=[], gemm_ms=[]) for label, _ in arms}
        for _ in range(reps + 1):
            for label, s in arms:
                wall, gemm, eff = self.call(fp32, form, m, n, k, dA, dB, dC, s)
                out[label]["S"] = eff
                out[label]["wall_ms"].append(round(wall, 3))
                out[label]["gemm_ms"].append(round(gemm, 3))
        if group == "sweep":      # compact: S -> repetitions, no warm-up
            return self.emit(dict(
                group=group, fp32=fp32, form=form, tiles=m * n // 16384, k=k,
                wall_ms={a["S"]: a["wall_ms"][1:] for a in out.values()}))
        self.emit(dict(group=group, fp32=fp32, form=form, m=m, n=n, k=k,
                       tiles=m * n // 16384, arms=out))


def sweep(b, reps, kmax, cap):
    """k = 512, 2048, .. (x4) and kmax itself; cap bounds one operand."""
    ks = [512 * 4 ** i for i in range(12) if 512 * 4 ** i < kmax] + [kmax]
    for fp32 in (0, 1):
        elem = 4 if fp32 else 8
        for name, seed in (("A", 0xA5), ("B", 0xB5)):   # the largest, once
            b.buf(name, min(cap, 2048 * kmax * elem), seed, fp32)
        for form in FORMS:
            for tiles, dim in TILE_DIMS.items():
                for k in ks:
                    if dim * k * elem > cap:
                        continue
                    top = min(resident(fp32, b.cus) // tiles, k // 16)
                    arms, s = [("plain", None)], 2
                    while s <= top:
                        arms.append((f"S{s}", s))
                        s *= 2
                    b.compare("sweep", fp32, form, dim, dim, k, arms, reps)


def report(b, reps):
    arms = [("plain", None), ("auto", 0)]
    b.compare("gram-2^20x1024-f64", 0, "tn", 1024, 1024, 1 << 20, arms, reps,
              same_ab=True)
    b.compare("gram-2^20x128-f64", 0, "tn", 128, 128, 1 << 20, arms, reps,
              same_ab=True)
    b.compare("512x512x131072-f64", 0, "nn", 512, 512, 131072, arms, reps)
    b.compare("512x512x131072-f32", 1, "nn", 512, 512, 131072, arms, reps)
    b.compare("8192^3-f64", 0, "nn", 8192, 8192, 8192, arms, reps)


def reduce_mode(b, reps):
    import numpy as np
    dim, vp = 4096, ctypes.c_void_p
    for fp32 in (0, 1):
        dt, elem = (np.float32, 4) if fp32 else (np.float64, 8)
        for s in (2, 4, 8):
            k = 16 * s
            dA = b.buf("A", dim * k * elem, 0xA5, fp32)
            dB = b.buf("B", dim * k * elem, 0xB5, fp32)
            dC = b.buf("C", dim * dim * elem, None, fp32)
            nmap = (s + 1) * dim * dim // 3
            x, y = np.ones(nmap, dtype=dt), np.ones(nmap, dtype=dt)
            z = np.empty(nmap, dtype=dt)
            split, mapped = [], []
            for _ in range(reps + 1):
                split.append(round(
                    b.call(fp32, "nn", dim, dim, k, dA, dB, dC, s)[1], 4))
                t0 = time.perf_counter()
                rc = b.E.lib().mx_map(b.eng._ctx, 0, fp32, nmap,
                                      x.ctypes.data_as(vp),
                                      y.ctypes.data_as(vp), 0.0,
                                      z.ctypes.data_as(vp))
                assert rc == 0, rc
                mapped.append(round((time.perf_counter() - t0) * 1e3, 3))
            b.emit(dict(group="reduce", fp32=fp32, S=s, m=dim, n=dim, k=k,
                        bytes=(s + 1) * dim * dim * elem, map_elems=nmap,
                        splitk_gemm_ms=split, map_wall_ms=mapped))


def trace_lines(path, label, reps, out):
    """The kernel durations (end - start, us, in dispatch order, the warm-up
    first) of splitk_reduce_kernel and map_kernel in a kernel trace of
    reduce_mode, one line per (type, S) as reduce_mode ran them."""
    import csv
    t = sorted(csv.DictReader(open(path)),
               key=lambda r: int(r["Start_Timestamp"]))
    outf = open(out, "a") if out else None
    for fp32, typ in ((0, "double"), (1, "float")):
        us = {}
        for kern in ("splitk_reduce_kernel", "map_kernel"):
            us[kern] = [
                round((int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
                      / 1e3, 1) for r in t
                if r["Kernel_Name"].startswith(f"void {kern}<{typ}>")]
            assert len(us[kern]) == 3 * (reps + 1), (kern, len(us[kern]))
        for i, s in enumerate((2, 4, 8)):
            lo, hi = i * (reps + 1), (i + 1) * (reps + 1)
            line = json.dumps(dict(
                group="reduce-trace", build=label, fp32=fp32, S=s,
                bytes=(s + 1) * 4096 * 4096 * (4 if fp32 else 8),
                reduce_kernel_us=us["splitk_reduce_kernel"][lo:hi],
                map_kernel_us=us["map_kernel"][lo:hi]))
            print(line)
            if outf:
                outf.write(line + "\n")


def analyze(path):
    rows = [json.loads(ln) for ln in open(path) if ln.startswith("{")]
    cus = next((r["cus"] for r in rows if r.get("group") == "device"), 256)
    table, spreads = {}, []          # (fp32, form, tiles, k, S) -> wall median
    for r in rows:
        if r.get("group") != "sweep":
            continue
        key = (r["fp32"], r["form"], r["tiles"], r["k"])
        for S, w in r["wall_ms"].items():
            table[key + (int(S),)] = statistics.median(w)
            if int(S) == 1:
                spreads.append((key, (max(w) - min(w)) / statistics.median(w)))
    sp = [s for _, s in spreads]
    print(f"# plain arm wall spread: median {statistics.median(sp) * 100:.1f}%"
          f" max {max(sp) * 100:.1f}%")
    # the auto rule of gemm_splitk_plan.h per candidate pair of constants;
    # the geomean is over every swept point, an unsplit one counting 1.0
    for div in (1, 2, 4):
        for cand in (4, 8, 16, 32, 64, 128):
            bad, picked, gain = [], 0, []
            for key, margin in spreads:
                fp32, _, tiles, k = key
                target = resident(fp32, cus) // div
                s = 1 if tiles >= target else max(
                    1, min(target // tiles, (k // 16) // cand))
                if s == 1 or key + (s,) not in table:
                    gain.append(1.0)
                    continue
                picked += 1
                plain, split = table[key + (1,)], table[key + (s,)]
                gain.append(plain / split)
                if split > plain * (1 + margin):
                    bad.append(key + (s, round(plain, 3), round(split, 3)))
            print(f"# fill resident/{div} MIN_KSTEPS {cand}: auto splits "
                  f"{picked} of {len(spreads)} points, geomean wall "
                  f"speed-up {statistics.geometric_mean(gain):.2f}x, slower "
                  f"than plain beyond its spread at {len(bad)}: {bad}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="sweep")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kmax", type=int, default=1 << 20)
    ap.add_argument("--operand-gib", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--analyze")
    ap.add_argument("--trace", help="rocprofv3 kernel trace csv of --mode "
                    "reduce: print its reduce-trace lines")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.analyze:
        return analyze(a.analyze)
    if a.trace:
        return trace_lines(a.trace, a.label, a.reps, a.out)
    b = Bench(a.out)
    try:
        b.emit(dict(group="device", cus=b.cus))
        for mode in a.mode.split(","):
            {"sweep": lambda: sweep(b, a.reps, a.kmax, a.operand_gib << 30),
             "report": lambda: report(b, a.reps),
             "reduce": lambda: reduce_mode(b, a.reps)}[mode]()
    finally:
        b.close()


if __name__ == "__main__":
    main()
