# Exact-arithmetic SUMMA panel-loop test helper (shared by
# test_gpu_summa_exact.py, summa_worker.py and the CPU-only
# test_exact_summa_inputs.py). Builds on _exact.py: the same exact_matrix
# data and the same bounds (K <= 512 fp32, K <= 4096 fp64). Accumulating
# across panels is still a sum of at most K products, so the
# representability argument of _exact.py covers the panel chain in any
# order and every comparison is exact equality.
#
# A global exact A (m x k), B (k x n) is cut into the per-position padded
# shard images of mx_*_summa_device, with the library's own slab split:
#   A_local (prow, j): roundup(mi,128) x kaj, pad rows ZERO (they reach
#                      C_local's pad rows, which must come out zero)
#   B_local (i, pcol): roundup(kbi,16) x nj, pad rows the NaN sentinel
#                      (correct code never reads them)
#   C_local          : roundup(mi,128) x roundup(nj,128), prefilled with
#                      the NaN sentinel (the loop must overwrite all of it)
# and every image carries one trailing guard column of the sentinel.
import functools
from collections import namedtuple

import numpy as np

import _exact
from _exact import UINT, _bits, _filled, _first_bad, _nan, dtype_of

SummaCase = namedtuple("SummaCase", "fp32 pr pc m k n kb")

GRIDS = [(1, 1), (2, 1), (2, 2), (4, 2), (2, 4), (3, 2)]
SHAPES = [
    (300, 500, 260),   # ragged everywhere
    (129, 509, 65),    # prime k: no slab cut is a multiple of 16
    (5, 300, 70),      # empty m-slabs at pr = 4
    (130, 5, 140),     # empty k-slabs: kbi == 0 for the last grid rows
]
WIDTHS = [48, 40, 16, 2048]
WIDTH_GRIDS = [(1, 1), (4, 2)]

# real one-rank entries: fp64 takes two panels at the default width 2048
REAL_SHAPES = {0: (200, 4000, 130), 1: (200, 500, 130)}
# child with MARLIN_SUMMA_KB=40
KNOB_KB = 40
KNOB_SHAPE = (300, 500, 260)


def roundup(x, a):
    return (x + a - 1) // a * a


def case_id(c):
    return (f"{'f32' if c.fp32 else 'f64'}-g{c.pr}x{c.pc}-"
            f"{c.m}x{c.k}x{c.n}-kb{c.kb}")


def virtual_cases():
    out = []
    for fp32 in (0, 1):
        for pr, pc in GRIDS:
            for m, k, n in SHAPES:
                out.append(SummaCase(fp32, pr, pc, m, k, n, 48))
        for pr, pc in WIDTH_GRIDS:
            for kb in WIDTHS:
                c = SummaCase(fp32, pr, pc, *SHAPES[0], kb)
                if c not in out:
                    out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def summa_inputs(fp32, m, k, n):
    """(A, B, ref, qa, qb): exact global operands, ref = A @ B in float64
    (computed once, never modified), and the int64 numerators."""
    assert k <= (_exact.F32_KMAX if fp32 else _exact.F64_KMAX)
    base = m * 1000003 + k * 10007 + n * 101 + fp32 * 7
    a, qa = _exact.exact_matrix(m, k, base + 0x5A00, fp32)
    b, qb = _exact.exact_matrix(k, n, base + 0x5B00, fp32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    for x in (a, b, ref):
        x.setflags(write=False)
    return a, b, ref, qa, qb


class Geometry:
    """Slab split of one grid position, from the library's mx_slab_*."""

    def __init__(self, c, prow, pcol):
        from marlin_amd import engine as E
        self.mi = E.slab_len(c.m, c.pr, prow)
        self.mo = E.slab_off(c.m, c.pr, prow)
        self.nj = E.slab_len(c.n, c.pc, pcol)
        self.no = E.slab_off(c.n, c.pc, pcol)
        self.mip, self.njp = roundup(self.mi, 128), roundup(self.nj, 128)
        self.empty = self.mi == 0 or self.nj == 0


def a_shard(c, prow, j, a=None):
    """Image of A_local at (prow, j): mip x (kaj + 1), or None where the
    shard has no rows or no k-columns. a: the global A to cut instead of
    the case's exact one (the rounding tests bring their own data)."""
    from marlin_amd import engine as E
    dt = dtype_of(c.fp32)
    if a is None:
        a = summa_inputs(c.fp32, c.m, c.k, c.n)[0]
    mi, mo = E.slab_len(c.m, c.pr, prow), E.slab_off(c.m, c.pr, prow)
    kaj, ko = E.slab_len(c.k, c.pc, j), E.slab_off(c.k, c.pc, j)
    if mi == 0 or kaj == 0:
        return None
    img = np.zeros((roundup(mi, 128), kaj + 1), dtype=dt, order="F")
    img[:mi, :kaj] = a[mo:mo + mi, ko:ko + kaj]
    img.view(UINT[dt])[:, kaj] = _exact.NAN_BITS[dt]
    return img


def b_shard(c, i, pcol, b=None):
    """Image of B_local at (i, pcol): roundup(kbi,16) x (nj + 1), pad rows
    and guard column the NaN sentinel; None where the shard is empty. b:
    the global B to cut instead of the case's exact one."""
    from marlin_amd import engine as E
    dt = dtype_of(c.fp32)
    if b is None:
        b = summa_inputs(c.fp32, c.m, c.k, c.n)[1]
    kbi, ko = E.slab_len(c.k, c.pr, i), E.slab_off(c.k, c.pr, i)
    nj, no = E.slab_len(c.n, c.pc, pcol), E.slab_off(c.n, c.pc, pcol)
    if kbi == 0 or nj == 0:
        return None
    img = _filled(roundup(kbi, 16), nj + 1, _nan(dt))
    img[:kbi, :nj] = b[ko:ko + kbi, no:no + nj]
    return img


def c_image(c, g):
    """C_local image of a position: mip x (njp + 1) of the sentinel. An
    empty position gets one sentinel column the entry must not touch."""
    dt = dtype_of(c.fp32)
    if g.empty:
        return _filled(128, 1, _nan(dt))
    return _filled(g.mip, g.njp + 1, _nan(dt))


def ref_block(c, g):
    ref = summa_inputs(c.fp32, c.m, c.k, c.n)[2]
    return ref[g.mo:g.mo + g.mi, g.no:g.no + g.nj]


def check_c_image(img, mi, nj, ref, sentinel_bits):
    """img: downloaded mip x (njp+1) C_local image. Same dict shape as
    _exact._check_image (pad_ok = guard column untouched), plus the pad
    contract of the device entries: pad rows and pad columns exactly 0."""
    njp = img.shape[1] - 1
    inner = img[:mi, :nj]
    first_bad = _first_bad(inner.astype(np.float64), ref)
    pad_rows = img[mi:, :njp]
    pad_cols = img[:, nj:njp]
    return {
        "ok": first_bad is None,
        "first_bad": first_bad,
        "sentinel_inside": bool((_bits(inner) == sentinel_bits).any()),
        "pad_ok": bool((_bits(img[:, njp:]) == sentinel_bits).all()),
        "pad_rows_zero": bool((pad_rows == 0).all()),
        "pad_cols_zero": bool((pad_cols == 0).all()),
    }


def _failed(rc):
    return {"ok": False, "rc": rc, "first_bad": None, "sentinel_inside": False,
            "pad_ok": False, "pad_rows_zero": False, "pad_cols_zero": False,
            "launches": -1, "comm_ms": -1.0}


def expected_launches(c, prow, pcol):
    """gemm_launches of one position: one per planned panel, 0 if empty."""
    from marlin_amd import engine as E
    if Geometry(c, prow, pcol).empty:
        return 0
    return len(E.plan_panels(c.k, c.pr, c.pc, c.kb))


# ---------------------------------------------------------------------------
# device runs
def _upload(eng, img, bufs):
    if img is None:
        return None
    return _exact._dev(eng, img, bufs)


def _finish(eng, dC, cimg, c, g, keep=None):
    """Download C, check it; result dict with launches / comm_ms."""
    dt = dtype_of(c.fp32)
    sent = _nan(dt).view(UINT[dt])
    got = np.empty_like(cimg)
    eng.download(got, dC, got.nbytes)
    st = eng.stats()
    if g.empty:
        res = {"ok": True, "first_bad": None, "sentinel_inside": False,
               "pad_ok": bool((_bits(got) == sent).all()),
               "pad_rows_zero": True, "pad_cols_zero": True}
    else:
        res = check_c_image(got, g.mi, g.nj, ref_block(c, g), sent)
    res.update(rc=0, launches=int(st["gemm_launches"]),
               comm_ms=float(st["comm_ms"]))
    if keep is not None:
        keep.append(got)
    return res


def run_virtual_case(eng, c, keep=None, kb_arg=None):
    """Every position of the case's grid through mx_gemm_summa_virtual.
    Shards are uploaded once per case. Returns {(prow, pcol): result};
    stops at the first HIP failure (rc -2). keep: list that receives the
    downloaded C images in position order. kb_arg: the kb_max argument
    where it differs from c.kb (0 = the entry's default width)."""
    from marlin_amd.engine import EngineError
    bufs, out = [], {}
    try:
        dA = {(i, j): _upload(eng, a_shard(c, i, j), bufs)
              for i in range(c.pr) for j in range(c.pc)}
        dB = {(i, j): _upload(eng, b_shard(c, i, j), bufs)
              for i in range(c.pr) for j in range(c.pc)}
        for prow in range(c.pr):
            for pcol in range(c.pc):
                g = Geometry(c, prow, pcol)
                cimg = c_image(c, g)
                dC = _exact._dev(eng, cimg, bufs)
                try:
                    eng.gemm_summa_virtual(
                        c.pr, c.pc, prow, pcol, c.m, c.k, c.n,
                        [dA[(prow, j)] for j in range(c.pc)],
                        [dB[(i, pcol)] for i in range(c.pr)],
                        dC, c.kb if kb_arg is None else kb_arg,
                        bool(c.fp32))
                except EngineError as e:
                    out[(prow, pcol)] = _failed(e.code)
                    if e.code == -2:
                        return out
                    continue
                out[(prow, pcol)] = _finish(eng, dC, cimg, c, g, keep)
        return out
    finally:
        for d in bufs:
            eng.free(d)


def kres_images(c):
    """Whole-k padded operand images of the k-resident device entry at
    1x1: A mip x (kp + 1), B kp x (njp + 1); the kernel reads every pad,
    so pads are zero and only the guard column holds the sentinel."""
    dt = dtype_of(c.fp32)
    a, b = summa_inputs(c.fp32, c.m, c.k, c.n)[:2]
    mip, njp, kp = roundup(c.m, 128), roundup(c.n, 128), roundup(c.k, 16)
    aimg = np.zeros((mip, kp + 1), dtype=dt, order="F")
    aimg[:c.m, :c.k] = a
    aimg.view(UINT[dt])[:, kp] = _exact.NAN_BITS[dt]
    bimg = np.zeros((kp, njp + 1), dtype=dt, order="F")
    bimg[:c.k, :c.n] = b
    bimg.view(UINT[dt])[:, njp] = _exact.NAN_BITS[dt]
    return aimg, bimg


def run_real_device(eng, c, entry, keep=None):
    """One real one-rank device entry (after comm_init(0, 1)) on the 1x1
    shards of case c. entry: 'summa' (mx_[ds]gemm_summa_device) or 'kres'
    (mx_gemm_summa_kres_device)."""
    from marlin_amd.engine import EngineError
    assert (c.pr, c.pc) == (1, 1)
    g = Geometry(c, 0, 0)
    cimg = c_image(c, g)
    bufs = []
    try:
        if entry == "kres":
            aimg, bimg = kres_images(c)
        else:
            aimg, bimg = a_shard(c, 0, 0), b_shard(c, 0, 0)
        dA, dB = _upload(eng, aimg, bufs), _upload(eng, bimg, bufs)
        dC = _exact._dev(eng, cimg, bufs)
        try:
            if entry == "kres":
                eng.gemm_summa_kres_device(c.m, c.k, c.n, dA, dB, dC,
                                           bool(c.fp32))
            elif c.fp32:
                eng.sgemm_summa_device(c.m, c.k, c.n, dA, dB, dC)
            else:
                eng.dgemm_summa_device(c.m, c.k, c.n, dA, dB, dC)
        except EngineError as e:
            return _failed(e.code)
        return _finish(eng, dC, cimg, c, g, keep)
    finally:
        for d in bufs:
            eng.free(d)


def run_real_host(eng, c, entry, keep=None, poison=None):
    """One real one-rank host entry on tight col-major operands: 'summa'
    (mx_[ds]gemm_summa) or 'kres' (mx_[ds]gemm_summa_kres). The host
    entries return the logical block only, so there are no pads to
    check. poison: called with the engine right before the entry, to
    dirty the cached workspaces the entry stages into."""
    import ctypes
    from marlin_amd import engine as E
    assert (c.pr, c.pc) == (1, 1)
    dt = dtype_of(c.fp32)
    a, b, ref = summa_inputs(c.fp32, c.m, c.k, c.n)[:3]
    got = _filled(c.m, c.n, _nan(dt))
    if poison is not None:
        poison(eng)
    name = "mx_%sgemm_summa%s" % ("s" if c.fp32 else "d",
                                  "_kres" if entry == "kres" else "")
    rc = getattr(E.lib(), name)(eng._ctx, c.m, c.k, c.n, E._fbuf(a, dt),
                                E._fbuf(b, dt), E._fbuf(got, dt))
    if rc != 0:
        return _failed(rc)
    st = eng.stats()
    first_bad = _first_bad(got.astype(np.float64), ref)
    sent = _nan(dt).view(UINT[dt])
    if keep is not None:
        keep.append(got)
    return {"ok": first_bad is None, "first_bad": first_bad,
            "sentinel_inside": bool((_bits(got) == sent).any()),
            "pad_ok": True, "pad_rows_zero": True, "pad_cols_zero": True,
            "rc": 0, "launches": int(st["gemm_launches"]),
            "comm_ms": float(st["comm_ms"])}
