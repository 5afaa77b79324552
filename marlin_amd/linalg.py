# linalg.py — the decomposition tier built on the GEMM engine:
# blocked LU and blocked inverse, restating the reference's distributed
# algorithms (DenseVecMatrix.luDecompose, DenseVecMatrix.scala:283-464;
# DenseVecMatrix.inverse, DenseVecMatrix.scala:565-764).
#
# Structure mirrors the reference exactly: the diagonal base block is
# factored on the HOST (the reference factors it on the Spark driver with
# Breeze LU/inv — a deliberate host step, not a fallback), and every
# panel scale and trailing-matrix update is a dense GEMM on the engine.
# All blocks stay DEVICE-RESIDENT (DeviceMatrix) across the sweeps —
# the RDD.cache() analog — so only the base-sized diagonal factors cross
# PCIe; sign flips are folded into the small host factors so no device
# elementwise pass is needed. cholesky_decompose(panel="trsm") and lu_solve
# instead use the device triangular solve (Engine.trsm_raw / trsm_dd): no
# inverse is formed and the factor is uploaded once. lu_factor_device goes
# further: the whole LU runs on the device (Engine.getrf_dd, pivoting inside
# 128-wide diagonal blocks) and the factor stays there for its solves.
#
# luDecompose: block pairwise pivoting (pivoting INSIDE each diagonal
# block only — the reference's scheme). Returns (blocks, p_array) with
# the property  P_blockdiag @ A == L @ U  (L unit-lower / U upper packed
# in the returned blocks; verified in tests).
# inverse: recursive block Gauss-Jordan; forward sweep stores
#   S1=A11^-1, S2=-A11^-1 A12, S3=-A21 A11^-1 and the Schur trailing
#   update; backward sweep recombines (DenseVecMatrix.scala:677-764).
import math

import numpy as np


def _split(n, base):
    nb = int(math.ceil(n / base))
    bl = int(math.ceil(n / nb))
    offs = [i * bl for i in range(nb)]
    lens = [min(bl, n - o) for o in offs]
    return nb, offs, lens


def _upload_blocks(eng, a, nb, offs, lens):
    return {(i, j): eng.upload_matrix(a[offs[i]:offs[i] + lens[i],
                                        offs[j]:offs[j] + lens[j]])
            for i in range(nb) for j in range(nb)}


def _gemm_batch(eng, problems, grouped, **kw):
    """A batch of mutually independent device GEMMs, (A, B, C) triples as
    Engine.gemm_grouped takes them: one grouped launch, or (grouped=False,
    the comparison arm) one launch and host sync per product. Both give
    the same bits. A batch of one has nothing to share a launch with and
    takes the plain entry either way. Returns the C handles."""
    if grouped and len(problems) > 1:
        return eng.gemm_grouped(problems, **kw)
    return [eng.gemm_dd(A, B, C, **kw) for A, B, C in problems]


class DeviceLU:
    """The packed L\\U factor of a square matrix, resident on the device,
    with its row permutation (A[p_array] == L @ U). Made by
    lu_factor_device; reusable for any number of solves; owns its image
    until free() (also the end of a `with` block)."""

    def __init__(self, eng, image, p_array):
        self._eng, self._image = eng, image
        self.p_array = p_array
        self.n = image.m
        self.fp32 = image.fp32

    def solve(self, rhs):
        """x with A x = rhs, a vector of n or an n x c matrix (its columns
        are padded to 128 on the device); the result has its shape and the
        factor's element type. The right-hand side is permuted on the host
        and uploaded; the factor is read where it lies, as unit-lower L and
        then as upper U (Engine.trsm_dd)."""
        if self._image is None:
            raise ValueError("DeviceLU used after free()")
        dt = np.float32 if self.fp32 else np.float64
        b = np.asarray(rhs, dtype=dt)
        if b.ndim not in (1, 2) or b.shape[0] != self.n:
            raise ValueError(
                f"right-hand side must have {self.n} rows: {b.shape}")
        pb = b.reshape(self.n, -1)[self.p_array, :]   # (P b)[g] = b[p[g]]
        d_b = self._eng.upload_matrix(pb, fp32=self.fp32)
        try:
            self._eng.trsm_dd(self._image, d_b, side="left", lower=True,
                              unit_diag=True)
            self._eng.trsm_dd(self._image, d_b, side="left", lower=False)
            x = self._eng.download_matrix(d_b)
        finally:
            d_b.free()
        return x[:, 0] if b.ndim == 1 else x

    def download(self):
        """(packed L\\U as an n x n ndarray, p_array)."""
        if self._image is None:
            raise ValueError("DeviceLU used after free()")
        return self._eng.download_matrix(self._image), self.p_array

    def free(self):
        """Releases the device image; a second call is a no-op."""
        if self._image is not None:
            self._image.free()
            self._image = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
        return False


def lu_factor_device(dvm, fp32=False):
    """LU of a square DenseVecMatrix wholly on the device: one upload, then
    Engine.getrf_dd (mx_getrf_device: a stream of launches, pivoting inside
    each 128 x 128 diagonal block, no host step). Returns a DeviceLU that
    keeps the packed factor on the device. Raises np.linalg.LinAlgError
    naming the column when a pivot is exactly zero. A matrix that needs a
    pivot from another block row is outside what block-local pivoting
    covers, here at width 128 as in lu_decompose at base_size."""
    a = dvm.toBreeze()
    if a.shape[0] != a.shape[1]:
        raise ValueError(
            f"LU decompose only support square matrix: {a.shape[0]} v.s "
            f"{a.shape[1]}")
    eng = dvm._engine()
    image = eng.upload_matrix(a, fp32=fp32)
    try:
        p_array, info = eng.getrf_dd(image)
        if info:
            raise np.linalg.LinAlgError(
                f"zero pivot in column {info} (1-based) of the block-pivoted "
                f"LU: U is singular")
    except BaseException:
        image.free()
        raise
    return DeviceLU(eng, image, p_array)


def lu_decompose(dvm, mode="auto", base_size=1000, grouped=True,
                 panel="host"):
    """DenseVecMatrix.luDecompose (DenseVecMatrix.scala:283-464).
    Returns (BlockMatrix with packed L\\U, p_array) where p_array[g] is
    the source row of output row g within its block row.
    panel="host" (the default) factors each diagonal base block on the
    host. panel="device" returns the same contract from
    lu_factor_device(dvm).download(): the whole factorisation runs on the
    device with pivoting inside 128-wide diagonal blocks, and mode,
    base_size and grouped play no part."""
    from .api import BlockMatrix
    import scipy.linalg

    if panel not in ("host", "device"):
        raise ValueError(f"panel must be 'host' or 'device': {panel!r}")
    if panel == "device":
        with lu_factor_device(dvm) as f:
            lu, p_array = f.download()
        n = lu.shape[0]
        return (BlockMatrix({(0, 0): lu}, n, n, engine=dvm._eng), p_array)
    a = dvm.toBreeze()
    n = a.shape[0]
    if a.shape[0] != a.shape[1]:
        raise ValueError(
            f"LU decompose only support square matrix: {a.shape[0]} v.s "
            f"{a.shape[1]}")
    if mode == "auto":
        mode = "dist" if n > 6000 else "local"
    if mode in ("local", "breeze"):
        lu, piv = scipy.linalg.lu_factor(a)
        p_array = np.arange(n)
        for i, p in enumerate(piv):
            p_array[i], p_array[p] = p_array[p], p_array[i]
        return (BlockMatrix({(0, 0): lu}, n, n, engine=dvm._eng), p_array)

    eng = dvm._engine()
    nb, offs, lens = _split(n, base_size)
    blk = _upload_blocks(eng, a, nb, offs, lens)
    host = {}                       # finished blocks, host-side
    p_array = np.arange(n)

    for i in range(nb):
        diag = eng.download_matrix(blk[(i, i)])
        lu, piv = scipy.linalg.lu_factor(diag)
        perm = np.arange(lens[i])
        for r, p in enumerate(piv):
            perm[r], perm[p] = perm[p], perm[r]
        p_array[offs[i]:offs[i] + lens[i]] = offs[i] + perm
        host[(i, i)] = lu                     # packed L\U of the diagonal
        if i == nb - 1:
            break
        L = np.tril(lu, -1) + np.eye(lens[i])
        U = np.triu(lu)
        P = np.zeros((lens[i], lens[i]))
        P[np.arange(lens[i]), perm] = 1.0     # row g of P·X is X[perm[g]]
        d_Minv = eng.upload_matrix(np.linalg.solve(L, P))     # L^-1 P
        d_negMinv = eng.upload_matrix(-np.linalg.solve(L, P))
        d_Uinv = eng.upload_matrix(np.linalg.inv(U))          # U^-1
        # panel scales + trailing update — device-resident GEMMs; the
        # scales of a step are one batch, its trailing update the next
        rest = range(i + 1, nb)
        scales = ([(d_negMinv, blk[(i, j)], None) for j in rest]  # -L^-1 P A12
                  + [(d_Minv, blk[(i, j)], None) for j in rest]   # U12 panel
                  + [(blk[(r, i)], d_Uinv, None) for r in rest])  # L21 panel
        done = _gemm_batch(eng, scales, grouped)
        nr = len(rest)
        negA2 = dict(zip(rest, done[:nr]))
        for j, new in zip(rest, done[nr:2 * nr]):
            blk[(i, j)].free()
            blk[(i, j)] = new
        for r, new in zip(rest, done[2 * nr:]):
            blk[(r, i)].free()
            blk[(r, i)] = new
        # A22 += L21 · (-U12)  (reference: A4 - A3 (A11 \\ A2))
        _gemm_batch(eng, [(blk[(r, i)], negA2[j], blk[(r, j)])
                          for r in rest for j in rest], grouped,
                    accumulate=True)
        for d in negA2.values():
            d.free()
        d_Minv.free(); d_negMinv.free(); d_Uinv.free()

    # materialise + sub-diagonal permutation fix-up
    # (DenseVecMatrix.scala:444-462): L21 block rows permuted by their
    # OWN block row's perm
    for (i, j), d in blk.items():
        if (i, j) not in host:
            host[(i, j)] = eng.download_matrix(d)
        d.free()
    for r in range(1, nb):
        perm = p_array[offs[r]:offs[r] + lens[r]] - offs[r]
        P = np.zeros((lens[r], lens[r]))
        P[np.arange(lens[r]), perm] = 1.0
        for c in range(r):
            host[(r, c)] = P @ host[(r, c)]
    return (BlockMatrix(host, n, n, engine=dvm._eng), p_array)


def inverse(dvm, mode="auto", base_size=1000, grouped=True):
    """DenseVecMatrix.inverse (DenseVecMatrix.scala:565-764)."""
    from .api import BlockMatrix

    a = dvm.toBreeze()
    n = a.shape[0]
    if a.shape[0] != a.shape[1]:
        raise ValueError("inverse only supports square matrices")
    if mode == "auto":
        mode = "dist" if n > 6000 else "local"
    if mode in ("local", "breeze"):
        # the reference's LocalBreeze route: driver-side inverse
        # (DenseVecMatrix.scala:585-590)
        inv = np.linalg.inv(a)
        return BlockMatrix({(0, 0): inv}, n, n, engine=dvm._eng)

    eng = dvm._engine()
    nb, offs, lens = _split(n, base_size)
    blk = _upload_blocks(eng, a, nb, offs, lens)
    S1, S2, S3 = {}, {}, {}

    # forward sweep (DenseVecMatrix.scala:604-675)
    for i in range(nb - 1):
        inv = np.linalg.inv(eng.download_matrix(blk[(i, i)]))
        S1[i] = inv
        d_inv = eng.upload_matrix(inv)
        d_neg = eng.upload_matrix(-inv)
        rest = range(i + 1, nb)
        done = _gemm_batch(
            eng, [(d_neg, blk[(i, j)], None) for j in rest]     # -A11^-1 A12
            + [(blk[(r, i)], d_neg, None) for r in rest],       # -A21 A11^-1
            grouped)
        for j, d in zip(rest, done[:len(rest)]):
            S2[(i, j)] = d
        for r, d in zip(rest, done[len(rest):]):
            S3[(r, i)] = d
        # A22 += A21 · (-A11^-1 A12)
        _gemm_batch(eng, [(blk[(r, i)], S2[(i, j)], blk[(r, j)])
                          for r in rest for j in rest], grouped,
                    accumulate=True)
        d_inv.free(); d_neg.free()
    last = eng.download_matrix(blk[(nb - 1, nb - 1)])
    T = {(nb - 1, nb - 1): eng.upload_matrix(np.linalg.inv(last))}

    # backward sweep (DenseVecMatrix.scala:677-764) — device-resident
    for i in range(nb - 2, -1, -1):
        # col[r] = sum_c T[r, c] S3[c, i] (inv[r, i]) and row[c] =
        # sum_j S2[i, j] T[j, c] (inv[i, c]): the chains are independent
        # of one another, so position t of every chain is one batch
        rest = range(i + 1, nb)
        col = dict.fromkeys(rest)
        row = dict.fromkeys(rest)
        for t in rest:
            done = _gemm_batch(
                eng, [(T[(r, t)], S3[(t, i)], col[r]) for r in rest]
                + [(S2[(i, t)], T[(t, c)], row[c]) for c in rest],
                grouped, accumulate=t > i + 1)
            col = dict(zip(rest, done[:len(rest)]))
            row = dict(zip(rest, done[len(rest):]))
        corner = eng.upload_matrix(S1[i])
        for j in range(i + 1, nb):
            eng.gemm_dd(S2[(i, j)], col[j], corner, accumulate=True)
        T[(i, i)] = corner
        for r in range(i + 1, nb):
            T[(r, i)] = col[r]
        for c in range(i + 1, nb):
            T[(i, c)] = row[c]

    out = {k: eng.download_matrix(d) for k, d in T.items()}
    for d in T.values():
        d.free()
    for d in list(S2.values()) + list(S3.values()) + list(blk.values()):
        d.free()
    return BlockMatrix(out, n, n, engine=dvm._eng)


def lu_solve(lu_blocks, p_array, rhs):
    """x with A x = rhs from the factors lu_decompose returned for A: the
    packed L\\U blocks and p_array, for which A[p_array, :] == L @ U, so
    that L U x = rhs[p_array]. The right-hand side is permuted on the host,
    the packed factor is uploaded ONCE and read twice as stored by the
    device triangular solve (Engine.trsm_dd): as unit-lower L, then as
    upper U. rhs is a vector of n or an n x c matrix (its columns are
    padded to 128 on the device); the result has its shape."""
    eng = lu_blocks._engine()
    lu = lu_blocks.toBreeze()
    n = lu.shape[0]
    b = np.asarray(rhs, dtype=np.float64)
    if b.ndim not in (1, 2) or b.shape[0] != n:
        raise ValueError(f"right-hand side must have {n} rows: {b.shape}")
    pb = b.reshape(n, -1)[np.asarray(p_array), :]   # (P b)[g] = b[p_array[g]]
    d_lu = eng.upload_matrix(lu)
    d_b = eng.upload_matrix(pb)
    try:
        eng.trsm_dd(d_lu, d_b, side="left", lower=True, unit_diag=True)
        eng.trsm_dd(d_lu, d_b, side="left", lower=False)
        x = eng.download_matrix(d_b)
    finally:
        d_lu.free()
        d_b.free()
    return x[:, 0] if b.ndim == 1 else x


def _r128(x):
    return (x + 127) // 128 * 128


def _cholesky_trsm(eng, a, nb, offs, lens):
    """The blocked sweep of cholesky_decompose(panel="trsm"). Block column
    j lives on the device as its diagonal block (a DeviceMatrix) and ONE
    panel image holding the blocks (j+1.., j) stacked, each padded to 128
    rows, so that the whole column panel is the B of a single right-side
    solve, L21 = A21 L11^-T, against the once-uploaded L11; its negated
    copy for the trailing update is an elementwise pass on the device, and
    the update's products address their blocks by offset into the panels.
    Returns the host blocks of the lower triangle."""
    rp = [_r128(ln) for ln in lens]
    top = [sum(rp[:i]) for i in range(nb + 1)]      # padded row of block i
    diag, panel, rows = {}, {}, {}
    # one host staging area for every panel image, up and down: a fresh
    # array per panel would be page-faulted in anew each time
    stage = np.zeros((top[nb] - top[1]) * max(rp))

    def image(j):
        return stage[:rows[j] * rp[j]].reshape((rows[j], rp[j]), order="F")
    for j in range(nb):
        diag[j] = eng.upload_matrix(a[offs[j]:offs[j] + lens[j],
                                      offs[j]:offs[j] + lens[j]])
        rows[j] = top[nb] - top[j + 1]              # pitch of panel j
        if rows[j] == 0:
            continue
        img = image(j)
        img[:, lens[j]:] = 0                        # the pads only
        for r in range(j + 1, nb):
            o = top[r] - top[j + 1]
            img[o + lens[r]:o + rp[r], :] = 0
            # block by block into column-major first: one strided pass over
            # a whole row-major column panel is several times slower
            img[o:o + lens[r], :lens[j]] = np.asfortranarray(
                a[offs[r]:offs[r] + lens[r], offs[j]:offs[j] + lens[j]])
        panel[j] = eng.alloc(img.nbytes)
        eng.upload(panel[j], img, img.nbytes)
    host = {}
    try:
        for i in range(nb):
            d = eng.download_matrix(diag[i])
            d = np.tril(d) + np.tril(d, -1).T       # symmetrize (ref does)
            L11 = np.linalg.cholesky(d)
            host[(i, i)] = L11
            if i == nb - 1:
                break
            d_L = neg = None
            try:
                d_L = eng.upload_matrix(L11)
                neg = eng.alloc(rows[i] * rp[i] * 8)
                # X L11^T = A21 over the whole panel: right, lower, trans
                eng.trsm_raw(lens[i], rows[i], d_L.buf, d_L.pitch, panel[i],
                             rows[i], side=1, lower=1, trans=1, unit_diag=0)
                eng.map_raw("muls", rows[i] * rp[i], panel[i], None, -1.0, neg)
                # A22[r, c] += L21[r] @ (-L21[c])^T, c <= r, as stored
                kp = (lens[i] + 15) // 16 * 16
                prods = []
                for c in range(i + 1, nb):
                    for r in range(c, nb):
                        cbuf, coff, ldc = ((diag[c].buf, 0, diag[c].pitch)
                                           if r == c else
                                           (panel[c], top[r] - top[c + 1],
                                            rows[c]))
                        prods.append((rp[r], kp, rp[c],
                                      panel[i], top[r] - top[i + 1], rows[i],
                                      neg, top[c] - top[i + 1], rows[i],
                                      cbuf, coff, ldc))
                eng.gemm_grouped_raw(prods, accumulate=True, trans_b=True)
            finally:
                if d_L is not None:
                    d_L.free()
                if neg is not None:
                    eng.free(neg)
        for j, buf in panel.items():
            img = image(j)
            eng.download(img, buf, img.nbytes)
            for r in range(j + 1, nb):
                o = top[r] - top[j + 1]
                host[(r, j)] = img[o:o + lens[r], :lens[j]].copy(order="F")
    finally:
        for d in diag.values():
            d.free()
        for buf in panel.values():
            eng.free(buf)
    return host


def cholesky_decompose(dvm, mode="auto", base_size=1000, grouped=True,
                       panel="inverse"):
    """DenseVecMatrix.choleskyDecompose (DenseVecMatrix.scala:475-566):
    A = L L^T, lower-triangular L. Right-looking blocked: host chol of
    the (symmetrized, as the reference does) diagonal block, panel scale
    L21 = A21 L11^-T and trailing A22 -= L21 L21^T as device-resident
    engine GEMMs. panel="inverse" (the default) scales the panel by the
    host inverse of L11, signs folded into the host factor;
    panel="trsm" solves it on the device instead (Engine.trsm_raw), with
    no inverse formed and L11 uploaded once."""
    from .api import BlockMatrix

    if panel not in ("inverse", "trsm"):
        raise ValueError(f"panel must be 'inverse' or 'trsm': {panel!r}")
    a = dvm.toBreeze()
    n = a.shape[0]
    if a.shape[0] != a.shape[1]:
        raise ValueError(
            f"LU decompose only support square matrix: {n} v.s {n}")
    if mode == "auto":
        mode = "dist" if n > 6000 else "local"
    if mode in ("local", "breeze"):
        L = np.linalg.cholesky(np.tril(a) + np.tril(a, -1).T)
        return BlockMatrix({(0, 0): L}, n, n, engine=dvm._eng)

    eng = dvm._engine()
    nb, offs, lens = _split(n, base_size)
    if panel == "trsm":
        host = _cholesky_trsm(eng, a, nb, offs, lens)
        for i in range(nb):
            for j in range(i + 1, nb):
                host[(i, j)] = np.zeros((lens[i], lens[j]))
        return BlockMatrix(host, n, n, engine=dvm._eng)
    blk = {(i, j): eng.upload_matrix(a[offs[i]:offs[i] + lens[i],
                                       offs[j]:offs[j] + lens[j]])
           for i in range(nb) for j in range(nb) if i >= j}
    host = {}
    for i in range(nb):
        diag = eng.download_matrix(blk[(i, i)])
        diag = np.tril(diag) + np.tril(diag, -1).T   # symmetrize (ref does)
        L11 = np.linalg.cholesky(diag)
        host[(i, i)] = L11
        if i == nb - 1:
            break
        linvT = np.linalg.inv(L11).T                 # L11^-T (host, base)
        d_pos = eng.upload_matrix(linvT)
        d_neg = eng.upload_matrix(-linvT)
        rest = range(i + 1, nb)
        done = _gemm_batch(
            eng, [(blk[(r, i)], d_pos, None) for r in rest]     # L21 panel
            + [(blk[(r, i)], d_neg, None) for r in rest],       # -L21
            grouped)
        neg = dict(zip(rest, done[len(rest):]))
        for r, l21 in zip(rest, done[:len(rest)]):
            blk[(r, i)].free()
            blk[(r, i)] = l21
        # A22 += L21[r] @ (-L21[c])^T, -L21[c] read as stored
        _gemm_batch(eng, [(blk[(r, i)], neg[c], blk[(r, c)])
                          for c in rest for r in range(c, nb)], grouped,
                    accumulate=True, trans_b=True)
        for d in neg.values():
            d.free()
        d_pos.free()
        d_neg.free()

    for (i, j), d in blk.items():
        if (i, j) not in host:
            host[(i, j)] = eng.download_matrix(d)
        d.free()
    # upper-triangle blocks are zero in the L result
    for i in range(nb):
        for j in range(i + 1, nb):
            host[(i, j)] = np.zeros((lens[i], lens[j]))
    # keep strictly-lower of diagonal factor only (chol returns lower)
    return BlockMatrix(host, n, n, engine=dvm._eng)
