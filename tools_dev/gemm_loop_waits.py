#!/usr/bin/env python3
# What the steady-state k-loop of every gemm_mfma_kernel instantiation
# waits for, read from a device-only assembly listing of kernels.hip
# (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S).
#
# Per kernel: the MFMA / VALU / SALU / ds_read / DMA / barrier / waitcnt
# counts of the loop body, VGPRs, scratch, LDS, occupancy, and for every
# `s_waitcnt lgkmcnt(n)` in the body its count operand and the number of
# MFMAs issued between the youngest ds_read that wait forces to complete
# and the wait itself. LDS operations return in order, so lgkmcnt(n)
# forces all but the n youngest; the body is walked twice so that a wait
# at the loop top sees the reads the previous iteration left in flight. A
# wait that forces nothing new (everything older was already waited for)
# has no distance. A wave that drains a read it issued 0..1 MFMAs earlier
# sits out an LDS round trip with nothing of its own queued on the matrix
# pipe; tests/test_gemm_loop_waits.py holds the pipelined loops to a
# minimum distance.
#
#   usage: gemm_loop_waits.py kernels.s            (markdown table)
#          gemm_loop_waits.py --compile [kernels.hip]
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS_HIP = os.path.join(os.path.dirname(HERE), "marlin_amd", "csrc",
                           "kernels.hip")
FIELDS = ("T", "BETA", "BK", "BM", "WM", "WN", "PIPE", "TA", "TB", "EPI",
          "GRP")


def compile_listing(src=KERNELS_HIP, out=None):
    """Device-only gfx950 assembly of src; returns the listing's path."""
    if out is None:
        out = os.path.join(tempfile.mkdtemp(prefix="gemm_asm_"), "kernels.s")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "--cuda-device-only", "-S", src, "-o", out], check=True,
                   capture_output=True)
    return out


def key_of(demangled):
    m = re.match(r"void gemm_mfma_kernel<([^>]*)>", demangled)
    if not m:
        return None
    a = [re.sub(r"^\(\w+\)", "", x.strip()) for x in m.group(1).split(",")]
    return tuple(a + ["0"] * (len(FIELDS) - len(a)))


def _instructions(body):
    ins = []
    for line in body.split("\n"):
        line = line.split(";")[0].strip()
        if re.match(r"\.LBB\d+_\d+:", line):
            ins.append(line)
        elif line and not line.startswith("."):
            ins.append(line)
    return ins


def loop_body(ins):
    """The steady-state k-loop: of the backward-branch spans that hold
    MFMAs and no other such span (a jump back to a block the layout put
    earlier spans whole loops and is none itself), the one with the most
    MFMAs."""
    pos = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
    spans = []
    for i, l in enumerate(ins):
        m = re.match(r"s_c?branch\w* (\.LBB\d+_\d+)", l)
        if not m or pos.get(m.group(1), i) >= i:
            continue
        lo = pos[m.group(1)]
        n = sum(1 for x in ins[lo:i + 1] if x.startswith("v_mfma_"))
        if n:
            spans.append((lo, i, n))
    inner = [s for s in spans
             if not any(t != s and s[0] <= t[0] and t[1] <= s[1]
                        for t in spans)]
    if not inner:
        return []
    lo, hi, _ = max(inner, key=lambda s: s[2])
    return ins[lo:hi + 1]


def classify(op):
    if op.startswith("v_mfma_"):
        return "mfma"
    if op.startswith("ds_read"):
        return "ds_read"
    if op.startswith("global_load_lds") or (
            op.startswith(("global_load", "buffer_load")) and " lds" in op):
        return "dma"
    if op.startswith("s_barrier"):
        return "barrier"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_") and not op.startswith(("s_nop", "s_cbranch",
                                                  "s_branch")):
        return "salu"
    return "other"


def lgkm_waits(body):
    """[(count operand, MFMA distance or None, after_barrier)] for every
    lgkmcnt wait of one pass over the body, in body order. after_barrier
    marks the first wait behind the s_barrier that forces a read: the
    loop-top wait on the next tile's quad-0 fragments."""
    out = []
    pending = []            # MFMA index at issue of every unforced ds_read
    mfmas = 0
    seen_barrier = False
    for rnd in (0, 1):
        for l in body:
            c = classify(l)
            if c == "mfma":
                mfmas += 1
            elif c == "ds_read":
                pending.append(mfmas)
            elif c == "barrier":
                seen_barrier = True
            elif c == "waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", l)
                if not m:
                    continue
                keep = min(int(m.group(1)), len(pending))
                n = int(m.group(1))
                forced = pending[:len(pending) - keep]
                dist = mfmas - forced[-1] if forced else None
                pending = pending[len(pending) - keep:]
                if rnd:
                    top = bool(forced) and seen_barrier
                    out.append((n, dist, top))
                if forced:
                    seen_barrier = False
    return out


def kernels(path):
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(names), text=True,
                         capture_output=True, check=True).stdout.split("\n")
    out = {}
    for name, d in zip(names, dem):
        k = key_of(d)
        if k is None:
            continue
        res = text.split("\n" + name + ":", 1)[1]
        ins = _instructions(res.split("\n", 1)[1].split(".Lfunc_end", 1)[0])
        meta = text.split(".amdhsa_kernel " + name + "\n", 1)[1]
        meta = meta.split(".end_amdhsa_kernel", 1)[0]

        def note(tag):
            return int(re.search(r"; " + tag + r": (\d+)", res).group(1))
        body = loop_body(ins)
        counts = {}
        for l in body:
            c = classify(l)
            counts[c] = counts.get(c, 0) + 1
        out[k] = dict(
            key=dict(zip(FIELDS, k)), counts=counts, waits=lgkm_waits(body),
            vgpr=note("TotalNumVgprs"), sgpr=note("TotalNumSgprs"),
            scratch=note("ScratchSize"), occ=note("Occupancy"),
            lds=int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)",
                              meta).group(1)))
    return out


def waits_text(waits):
    return " ".join(f"({n}):{'-' if d is None else d}{'^' if top else ''}"
                    for n, d, top in waits)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--compile":
        path = compile_listing(*(args[1:2] or [KERNELS_HIP]))
    else:
        path = args[0]
    ks = kernels(path)
    cols = ("mfma", "valu", "salu", "ds_read", "dma", "barrier", "waitcnt")
    print("| kernel <" + ",".join(FIELDS) + "> | " + " | ".join(cols) +
          " | VGPR | scratch | LDS | occ | lgkmcnt waits (n):MFMAs since "
          "the youngest forced read, ^ = loop-top wait |")
    print("|---" * (len(cols) + 6) + "|")
    for k in sorted(ks):
        r = ks[k]
        print(f"| {','.join(k)} | " +
              " | ".join(str(r["counts"].get(c, 0)) for c in cols) +
              f" | {r['vgpr']} | {r['scratch']} | {r['lds']} | {r['occ']} | "
              f"{waits_text(r['waits'])} |")


if __name__ == "__main__":
    main()
