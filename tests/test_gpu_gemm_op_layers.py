# Transposed-operand multiply above the ABI: Engine.gemm_dd on ragged
# device-resident matrices, Engine.dgemm / sgemm through mx_gemm_op, and
# the two consumers that used to hold a transposed copy
# (computeGramianMatrix, the Cholesky trailing update). Checked against
# numpy fp64 at the project's bars: <= 1e-10 relative for fp64, <= 1e-4
# for fp32.
import numpy as np
import pytest

from marlin_amd import DenseVecMatrix, Engine
from oracle import gen_matrix

pytestmark = pytest.mark.gpu

BAR = {False: 1e-10, True: 1e-4}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rel(got, ref):
    return np.max(np.abs(got.astype(np.float64) - ref)) / np.max(np.abs(ref))


def _op(x, t):
    return x.T if t else x


# stored shapes of (A, B) per form
DD_CASES = {
    "tn-gram": ((300, 70), None, True, False),          # A^T·A, one image
    "nt": ((130, 45), (200, 45), False, True),
    "tt": ((45, 130), (200, 45), True, True),
    "tn": ((301, 70), (301, 150), True, False),
}


@pytest.mark.parametrize("fp32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(DD_CASES))
def test_gemm_dd_transposed_forms(eng, name, fp32):
    sa, sb, ta, tb = DD_CASES[name]
    a = gen_matrix(*sa, seed=0x7A00 + len(name))
    b = a if sb is None else gen_matrix(*sb, seed=0x7B00 + len(name))
    dA = eng.upload_matrix(a, fp32=fp32)
    dB = dA if sb is None else eng.upload_matrix(b, fp32=fp32)
    try:
        C = eng.gemm_dd(dA, dB, trans_a=ta, trans_b=tb)
        assert eng.last_gemm_op() == (int(ta), int(tb))
        ref = _op(a, ta) @ _op(b, tb)
        assert (C.m, C.n) == ref.shape
        assert C.pitch == (ref.shape[0] + 127) // 128 * 128
        got = eng.download_matrix(C)
        C.free()
        assert _rel(got, ref) <= BAR[fp32]
    finally:
        dA.free()
        if dB is not dA:
            dB.free()


def test_gemm_dd_accumulate_transposed(eng):
    a = gen_matrix(130, 45, seed=0x7C01)
    b = gen_matrix(200, 45, seed=0x7C02)
    a2 = gen_matrix(33, 130, seed=0x7C03)
    b2 = gen_matrix(33, 200, seed=0x7C04)
    ds = [eng.upload_matrix(x) for x in (a, b, a2, b2)]
    try:
        C = eng.gemm_dd(ds[0], ds[1], trans_b=True)                # A·B^T
        C2 = eng.gemm_dd(ds[2], ds[3], C, accumulate=True, trans_a=True)
        assert C2 is C and eng.last_gemm_op() == (1, 0)
        got = eng.download_matrix(C)
        C.free()
        assert _rel(got, a @ b.T + a2.T @ b2) <= BAR[False]
    finally:
        for d in ds:
            d.free()


def test_gemm_dd_result_feeds_next_gemm_and_has_zero_pads(eng):
    """G = A^T·A, then G·G (NN): C's pad region must be exactly zero for
    the padded-dim GEMM that follows to stay exact."""
    a = gen_matrix(300, 70, seed=0x7D01)
    dA = eng.upload_matrix(a)
    try:
        G = eng.gemm_dd(dA, dA, trans_a=True)
        # the whole padded image, once: 128 x 128 for the 70 x 70 result
        ncap = (G.n + 127) // 128 * 128
        img = np.empty((G.pitch, ncap), dtype=np.float64, order="F")
        eng.download(img, G.buf, img.nbytes)
        g = a.T @ a
        assert _rel(img[:70, :70], g) <= BAR[False]
        pad = img.copy()
        pad[:70, :70] = 0
        assert not pad.any(), "pad region of C is not exactly zero"
        GG = eng.gemm_dd(G, G)
        assert eng.last_gemm_op() == (0, 0)
        got = eng.download_matrix(GG)
        GG.free()
        G.free()
        assert _rel(got, g @ g) <= BAR[False]
    finally:
        dA.free()


@pytest.mark.parametrize("ta,tb", [(False, False), (True, False),
                                   (False, True), (True, True)])
def test_gemm_dd_dimension_mismatch(eng, ta, tb):
    # inner dims 45 vs 46 under every form
    sa = (45, 130) if ta else (130, 45)
    sb = (200, 46) if tb else (46, 200)
    dA = eng.upload_matrix(np.ones(sa))
    dB = eng.upload_matrix(np.ones(sb))
    try:
        with pytest.raises(ValueError, match="Dimension mismatch during "
                                             "matrix-matrix multiplication"):
            eng.gemm_dd(dA, dB, trans_a=ta, trans_b=tb)
    finally:
        dA.free()
        dB.free()


def test_host_dgemm_sgemm_transposed(eng):
    a = gen_matrix(517, 301, seed=0xA11CE)
    b = gen_matrix(301, 733, seed=0xB0B)
    ref = a @ b
    at, bt = np.asfortranarray(a.T), np.asfortranarray(b.T)
    c = eng.dgemm(at, b, trans_a=True)                   # A stored 301 x 517
    assert eng.last_gemm_op() == (1, 0)
    assert c.shape == ref.shape and c.dtype == np.float64
    assert _rel(c, ref) <= BAR[False]
    c = eng.dgemm(at, bt, trans_a=True, trans_b=True)
    assert eng.last_gemm_op() == (1, 1)
    assert _rel(c, ref) <= BAR[False]
    c = eng.sgemm(a, bt, trans_b=True)                   # B stored 733 x 301
    assert eng.last_gemm_op() == (0, 1)
    assert c.shape == ref.shape and c.dtype == np.float32
    assert _rel(c, ref) <= BAR[True]
    with pytest.raises(ValueError, match="Dimension mismatch"):
        eng.dgemm(a, b, trans_a=True)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        eng.sgemm(a, b, trans_b=True)
    # the defaults keep the plain call
    assert _rel(eng.dgemm(a, b), ref) <= BAR[False]
    assert eng.last_gemm_op() == (0, 0)


# ---------------------------------------------------------------------------
# consumers
def test_gramian_reads_the_one_image(eng):
    a = gen_matrix(500, 90, seed=0x6A01)
    g = DenseVecMatrix(a, engine=eng).computeGramianMatrix()
    assert g.shape == (90, 90)
    assert _rel(g, a.T @ a) <= 1e-10
    assert eng.last_gemm_op() == (1, 0)


def test_cholesky_trailing_update_reads_l21_as_stored(eng):
    n = 300
    r = gen_matrix(n, n, seed=2000 + n)
    a = (r + r.T) / 2 + n * np.eye(n)
    L = DenseVecMatrix(a, engine=eng).choleskyDecompose(
        mode="dist", base_size=128).toBreeze()
    assert eng.last_gemm_op() == (0, 1)
    assert np.allclose(np.triu(L, 1), 0)
    rel = np.max(np.abs(L @ L.T - a)) / np.max(np.abs(a))
    assert rel < 1e-12, rel
