#!/usr/bin/env python3
# Compare the GEMM kernels of two device-only assembly listings of
# kernels.hip (hipcc --offload-arch=gfx950 -O3 -std=c++17
# --cuda-device-only -S): per kernel, instruction count old/new, whether
# the instruction streams are identical, the resource metadata, and the
# MFMA / LDS-read / DMA / barrier / waitcnt counts of the k-loop body.
# Prints one markdown table.   usage: cmp_gemm_asm.py parent.s new.s
import re
import subprocess
import sys

CLASSES = (("mfma", r"v_mfma_"), ("lds_rd", r"ds_read"),
           ("dma", r"global_load_lds"), ("barrier", r"s_barrier"),
           ("waitcnt", r"s_waitcnt"))


def key_of(demangled):
    # gemm_mfma_kernel<T, BETA, BK, BM, WM, WN, PIPE, TA, TB[, EPI[, GRP]]>
    m = re.match(r"void gemm_mfma_kernel<([^>]*)>", demangled)
    if m:
        a = [x.strip() for x in m.group(1).split(",")]
        a = [re.sub(r"^\(\w+\)", "", x) for x in a]     # (EPI)1 -> 1
        a += ["0"] * (11 - len(a))
        return tuple(a)
    if demangled.startswith("sgemm_mfma_tn_epilogue_kernel"):
        return ("float", "0", "16", "128", "2", "2", "0", "0", "0", "1", "0")
    return None


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
        body = res.split("\n", 1)[1].split(".Lfunc_end", 1)[0]
        ins = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                if re.match(r"\.LBB\d+_\d+:", line):
                    ins.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
                continue
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
        meta = text.split(".amdhsa_kernel " + name + "\n", 1)[1]
        meta = meta.split(".end_amdhsa_kernel", 1)[0]

        def note(tag):
            return re.search(r"; " + tag + r": (\d+)", res).group(1)
        out[k] = dict(
            ins=ins, n=sum(1 for i in ins if not i.endswith(":")),
            vgpr=note("TotalNumVgprs"), sgpr=note("TotalNumSgprs"),
            scratch=note("ScratchSize"), occ=note("Occupancy"),
            lds=re.search(r"\.amdhsa_group_segment_fixed_size (\d+)",
                          meta).group(1),
            loop=loop_counts(ins))
    return out


def loop_counts(ins):
    # k-loop body: the backward-branch span that holds the most MFMAs,
    # grown over blocks the layout put before or after it (a block the
    # span jumps back to, or jumps out to and returns from)
    pos = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
    br = {}
    for i, l in enumerate(ins):
        m = re.match(r"s_c?branch\w* (\.LBB_\d+)", l)
        if m and m.group(1) in pos:
            br[i] = pos[m.group(1)]
    best = None
    for i, j in br.items():
        if j >= i:
            continue
        lo, hi, grown = j, i, True
        while grown:
            grown = False
            for q, p in br.items():
                if lo <= q <= hi and p < lo:
                    lo, grown = p, True
                if q > hi and lo <= p <= hi and any(
                        lo <= q2 <= hi and hi < p2 <= q
                        for q2, p2 in br.items()):
                    hi, grown = q, True
        c = tuple(sum(1 for x in ins[lo:hi] if re.match(rx, x))
                  for _, rx in CLASSES)
        if best is None or (c[0], hi - lo) > (best[0][0], best[1]):
            best = (c, hi - lo)
    return best[0] if best else (0,) * len(CLASSES)


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    # a kernel only the new listing has (a new instantiation family) is
    # shown against its twin with the trailing GRP argument cleared
    assert set(old) <= set(new), set(old) - set(new)
    added = sorted(set(new) - set(old))
    print("| kernel <T,BETA,BK,BM,WM,WN,PIPE,TA,TB,EPI,GRP> | instr old/new | "
          "identical | VGPR | SGPR | scratch | LDS | occ | loop "
          + "/".join(n for n, _ in CLASSES) + " |")
    print("|---|---|---|---|---|---|---|---|---|")
    bad = 0
    for k in sorted(old):
        o, n = old[k], new[k]
        same = o["ins"] == n["ins"]

        def pair(f):
            return o[f] if o[f] == n[f] else f"{o[f]}->{n[f]}"
        loop = "/".join(map(str, n["loop"]))
        if o["loop"] != n["loop"]:
            loop = "/".join(map(str, o["loop"])) + " -> " + loop
        def per_step(c):
            # a body unrolled by two k-steps holds 128 MFMAs: compare the
            # MFMA / DMA / barrier counts of one step
            steps = max(1, c[0] // 64)
            return [c[i] / steps for i in (0, 2, 3)]
        if (int(n["scratch"]) > int(o["scratch"]) or
                int(n["occ"]) < int(o["occ"]) or
                per_step(o["loop"]) != per_step(n["loop"])):
            bad += 1
            loop += " **FAIL**"
        print(f"| {','.join(k)} | {o['n']}/{n['n']} | "
              f"{'yes' if same else 'no'} | {pair('vgpr')} | {pair('sgpr')} | "
              f"{pair('scratch')} | {pair('lds')} | {pair('occ')} | {loop} |")
    for k in added:
        n, t = new[k], new.get(k[:-1] + ("0",))
        loop = "/".join(map(str, n["loop"]))
        twin = "no twin"
        if t:
            twin = ("twin loop equal" if t["loop"] == n["loop"] else
                    "twin loop " + "/".join(map(str, t["loop"])))
            twin += f", twin instr {t['n']} VGPR {t['vgpr']} SGPR {t['sgpr']}"
        print(f"| {','.join(k)} | new/{n['n']} | new | {n['vgpr']} | "
              f"{n['sgpr']} | {n['scratch']} | {n['lds']} | {n['occ']} | "
              f"{loop} ({twin}) |")
    ident = sum(old[k]["ins"] == new[k]["ins"] for k in old)
    print(f"\n{len(old)} kernels, {ident} identical, {len(added)} new, "
          f"{bad} failing a "
          "condition (scratch up, occupancy down, loop MFMA/DMA/barrier "
          "counts changed)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
