# Transposed-operand GEMM against the parent build (diagnostics only).
#
#   python tools_dev/bench_gemm_op.py PARENT.so NEW.so [--reps 5] [--out F]
#       [--arms gemm64,gemm32,gram,chol] [--n 16384]
#
# PARENT.so is the parent commit's libmarlin_gpu.so (no mx_gemm_device_op),
# NEW.so this tree's. Each library lives in its own worker process (this
# file run with --worker), both alive for the whole run; the driver itself
# never opens the GPU and alternates the arms measurement by measurement,
# so every comparison is between runs interleaved on one device. Operands
# are device-resident. GEMM-only arms report the hipEvent kernel time of
# mx_stats; the end-to-end arms a host clock around the synchronising
# entries, with every buffer allocated beforehand. One warm-up per arm and
# shape, then --reps alternated repetitions. Every measurement is printed
# as one JSON line in run order (and appended to --out), then medians.
import argparse
import ctypes
import json
import statistics
import subprocess
import sys
import time

i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p


class Stats(ctypes.Structure):
    _fields_ = [(f, ctypes.c_double) for f in (
        "h2d_ms", "d2h_ms", "pack_ms", "gemm_ms", "comm_ms", "total_ms")] + [
        ("gemm_launches", i64), ("flops", ctypes.c_double),
        ("bytes_moved", ctypes.c_double)]


def up(x, a):
    return (x + a - 1) // a * a


class Worker:
    def __init__(self, so):
        self.lib = lib = ctypes.CDLL(so)
        lib.mx_init.argtypes = [ctypes.POINTER(vp), ci]
        lib.mx_alloc.argtypes = [vp, i64, ctypes.POINTER(vp)]
        lib.mx_free.argtypes = [vp, vp]
        lib.mx_memset.argtypes = [vp, vp, i64]
        lib.mx_fill_random.argtypes = [vp, vp, i64, ctypes.c_uint64, ci]
        lib.mx_stats.argtypes = [vp, ctypes.POINTER(Stats)]
        lib.mx_transpose_device.argtypes = [vp, ci, i64, i64, vp, vp]
        g = [vp, ci, ci, i64, i64, i64, vp, i64, vp, i64, vp, i64]
        lib.mx_gemm_device_ex.argtypes = g
        self.has_op = hasattr(lib, "mx_gemm_device_op")
        if self.has_op:
            lib.mx_gemm_device_op.argtypes = g[:3] + [ci, ci] + g[3:]
        self.ctx = vp()
        assert lib.mx_init(ctypes.byref(self.ctx), 0) == 0
        self.bufs = {}

    def alloc(self, name, elems, elem, seed=None, fp32=0):
        b = vp()
        assert self.lib.mx_alloc(self.ctx, elems * elem, ctypes.byref(b)) == 0
        if seed is None:
            assert self.lib.mx_memset(self.ctx, b, elems * elem) == 0
        else:
            assert self.lib.mx_fill_random(self.ctx, b, elems, seed, fp32) == 0
        self.bufs[name] = b
        return b

    def free_all(self):
        for b in self.bufs.values():
            self.lib.mx_free(self.ctx, b)
        self.bufs = {}

    def gemm(self, fp32, beta, ta, tb, m, k, n, a, lda, b, ldb, c, ldc):
        A, B, C = (self.bufs[x] for x in (a, b, c))
        if ta or tb:
            rc = self.lib.mx_gemm_device_op(self.ctx, fp32, beta, ta, tb, m,
                                            k, n, A, lda, B, ldb, C, ldc)
        else:
            rc = self.lib.mx_gemm_device_ex(self.ctx, fp32, beta, m, k, n, A,
                                            lda, B, ldb, C, ldc)
        assert rc == 0, rc
        st = Stats()
        self.lib.mx_stats(self.ctx, ctypes.byref(st))
        return st.gemm_ms

    def transpose(self, m, n, src, dst):
        assert self.lib.mx_transpose_device(self.ctx, 0, m, n, self.bufs[src],
                                            self.bufs[dst]) == 0

    # -- commands -----------------------------------------------------------
    def setup_gemm(self, fp32, n):
        self.free_all()
        elem = 4 if fp32 else 8
        self.alloc("A", n * n, elem, 1, fp32)
        self.alloc("B", n * n, elem, 2, fp32)
        self.alloc("C", n * n, elem)
        return {}

    def run_gemm(self, fp32, n, ta, tb):
        # square: the same two images serve every form
        ms = self.gemm(fp32, 0, ta, tb, n, n, n, "A", n, "B", n, "C", n)
        return {"ms": ms, "tflops": 2.0 * n ** 3 / ms / 1e9}

    def setup_gram(self, m, n):
        self.free_all()
        self.gm, self.gn = up(m, 128), up(n, 128)
        self.alloc("A", self.gm * self.gn, 8, 3)
        self.alloc("G", self.gn * self.gn, 8)
        self.alloc("AT", self.gn * self.gm, 8)   # used by the copy path only
        return {}

    def run_gram(self, path):
        mp, np_ = self.gm, self.gn
        t0 = time.perf_counter()
        if path == "copy":       # parent: transposed copy, then NN
            self.transpose(mp, np_, "A", "AT")
            self.gemm(0, 0, 0, 0, np_, mp, np_, "AT", np_, "A", mp, "G", np_)
        else:                    # new: A^T·A on the one image
            self.gemm(0, 0, 1, 0, np_, mp, np_, "A", mp, "A", mp, "G", np_)
        ms = (time.perf_counter() - t0) * 1e3
        return {"ms": ms, "tflops": 2.0 * mp * np_ * np_ / ms / 1e9}

    def setup_chol(self, b, nt):
        """One Cholesky panel step: nt trailing block rows of size b."""
        self.free_all()
        self.cb, self.cnt = b, nt
        self.alloc("Dn", b * b, 8, 4)
        for r in range(nt):
            self.alloc(f"old{r}", b * b, 8, 10 + r)
            self.alloc(f"neg{r}", b * b, 8)
            self.alloc(f"negT{r}", b * b, 8)
            for c in range(r + 1):
                self.alloc(f"blk{r}_{c}", b * b, 8)
        return {}

    def run_chol(self, path):
        b, nt = self.cb, self.cnt
        t0 = time.perf_counter()
        for r in range(nt):
            self.gemm(0, 0, 0, 0, b, b, b, f"old{r}", b, "Dn", b, f"neg{r}", b)
            if path == "copy":
                self.transpose(b, b, f"neg{r}", f"negT{r}")
        for c in range(nt):
            for r in range(c, nt):
                if path == "copy":
                    self.gemm(0, 1, 0, 0, b, b, b, f"old{r}", b, f"negT{c}",
                              b, f"blk{r}_{c}", b)
                else:
                    self.gemm(0, 1, 0, 1, b, b, b, f"old{r}", b, f"neg{c}",
                              b, f"blk{r}_{c}", b)
        return {"ms": (time.perf_counter() - t0) * 1e3}


def worker_main(so):
    w = Worker(so)
    print(json.dumps({"ready": True, "has_op": w.has_op}), flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        if req["cmd"] == "quit":
            break
        out = getattr(w, req["cmd"])(*req.get("args", []))
        print(json.dumps(out), flush=True)
    w.free_all()


class Remote:
    def __init__(self, name, so):
        self.name = name
        self.p = subprocess.Popen([sys.executable, __file__, "--worker", so],
                                  stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True)
        self.info = json.loads(self.p.stdout.readline())

    def call(self, cmd, *args):
        self.p.stdin.write(json.dumps({"cmd": cmd, "args": list(args)}) + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError(f"{self.name} worker died in {cmd}")
        return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write('{"cmd": "quit"}\n')
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_so")
    ap.add_argument("new_so")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--gram", default="40000x8192")
    ap.add_argument("--chol", default="2048x3")
    ap.add_argument("--arms", default="gemm64,gemm32,gram,chol")
    ap.add_argument("--out")
    a = ap.parse_args()
    par, new = Remote("parent", a.parent_so), Remote("new", a.new_so)
    assert not par.info["has_op"] and new.info["has_op"]
    outf = open(a.out, "a") if a.out else None
    rows = []

    def record(group, arm, rep, res):
        rec = dict(group=group, arm=arm, rep=rep, **res)
        rows.append(rec)
        line = json.dumps(rec)
        print(line, flush=True)
        if outf:
            outf.write(line + "\n")
            outf.flush()

    def run(group, arms):
        """arms: [(label, remote, cmd, args)]; rep -1 is the warm-up."""
        for rep in range(-1, a.reps):
            for label, rem, cmd, args in arms:
                record(group, label, rep, rem.call(cmd, *args))

    try:
        for fp32 in (0, 1):
            key = "gemm32" if fp32 else "gemm64"
            if key not in a.arms:
                continue
            for r in (par, new):
                r.call("setup_gemm", fp32, a.n)
            arms = [("parent-nn", par, "run_gemm", [fp32, a.n, 0, 0])]
            arms += [(f"new-{'nt'[ta]}{'nt'[tb]}", new, "run_gemm",
                      [fp32, a.n, ta, tb])
                     for ta, tb in ((0, 0), (1, 0), (0, 1), (1, 1))]
            run(f"{key}-{a.n}", arms)
        if "gram" in a.arms:
            m, n = (int(x) for x in a.gram.split("x"))
            for r in (par, new):
                r.call("setup_gram", m, n)
            run(f"gram-{a.gram}", [("parent-copy+nn", par, "run_gram", ["copy"]),
                                   ("new-tn", new, "run_gram", ["tn"])])
        if "chol" in a.arms:
            b, nt = (int(x) for x in a.chol.split("x"))
            for r in (par, new):
                r.call("setup_chol", b, nt)
            run(f"chol-step-{a.chol}",
                [("parent-copy+nn", par, "run_chol", ["copy"]),
                 ("new-nt", new, "run_chol", ["nt"])])
    finally:
        par.close()
        new.close()
    print("# medians (warm-up excluded): group arm median_ms min max "
          "(max-min)/median")
    seen = []
    for r in rows:
        if (r["group"], r["arm"]) not in seen:
            seen.append((r["group"], r["arm"]))
    for g, arm in seen:
        ms = [r["ms"] for r in rows
              if (r["group"], r["arm"]) == (g, arm) and r["rep"] >= 0]
        med = statistics.median(ms)
        line = (f"# {g} {arm} {med:.3f} {min(ms):.3f} {max(ms):.3f} "
                f"{(max(ms) - min(ms)) / med * 100:.2f}%")
        print(line)
        if outf:
            outf.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        worker_main(sys.argv[2])
    else:
        main()
