# Exact GPU tests of the auxiliary kernels (fill_random, zero_pad, map,
# sum, transpose, gemv) and of the argument checks of their entries.
# Everything is compared bit for bit (view(uint32/uint64) +
# assert_array_equal); there is no tolerance in this module. Why the
# expected values are exact is stated in tests/_aux_cases.py and asserted
# from the generated data in tests/test_aux_cases.py.
#
# Device buffers are uploaded from host images in which every element
# outside the logical operand is the NaN sentinel of _exact.NAN_BITS; after
# the call the whole buffer comes back and everything outside the region
# the call may write must be unchanged.
import ctypes

import numpy as np
import pytest

import _aux_cases as AC
import _exact
from _aux_cases import bits, nan_of, sentinel_vector, with_tail
from _exact import UINT, dtype_of
from marlin_amd import Engine
from marlin_amd import engine as E

pytestmark = pytest.mark.gpu

EINVAL = -4
FP = pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Bufs:
    """Device buffers of one test, each remembered with its host image."""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def put(self, img):
        d = self.eng.alloc(img.nbytes)
        self.held.append((d, img))
        self.eng.upload(d, img, img.nbytes)
        return d

    def get(self, d):
        img = next(i for h, i in self.held if h is d)
        got = np.empty_like(img)
        self.eng.download(got, d, got.nbytes)
        return got

    def assert_untouched(self):
        for d, img in self.held:
            np.testing.assert_array_equal(bits(self.get(d)), bits(img))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d, _ in self.held:
            self.eng.free(d)


def _assert_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------
# gemv
@pytest.mark.parametrize("m,n,lda", AC.GEMV_SHAPES)
def test_gemv_device_exact(eng, m, n, lda):
    _, x, _, _, ref = AC.gemv_inputs(m, n)
    with Bufs(eng) as bufs:
        dA = bufs.put(AC.gemv_device_image(m, n, lda))
        y = eng.dgemv_device_raw(m, n, dA, lda, x)
        _assert_bits(y, ref)
        bufs.assert_untouched()


@pytest.mark.parametrize("m,n,lda", AC.GEMV_SHAPES)
def test_gemv_host_exact(eng, m, n, lda):
    a, x, _, _, ref = AC.gemv_inputs(m, n)
    _assert_bits(eng.dgemv(a, x), ref)


# ---------------------------------------------------------------------------
# sum
@FP
@pytest.mark.parametrize("n", AC.SUM_NS)
def test_sum_exact(eng, n, fp32):
    vals, _, expected = AC.sum_inputs(n, fp32)
    out = ctypes.c_double(float("nan"))
    rc = E.lib().mx_sum(eng._ctx, fp32, n, _vp(vals), ctypes.byref(out))
    assert rc == 0
    _assert_bits(np.float64(out.value).reshape(1),
                 np.float64(expected).reshape(1))


# ---------------------------------------------------------------------------
# transpose
def _transposed(a):
    return np.asfortranarray(a.T)


@FP
@pytest.mark.parametrize("m,n", AC.TRANSPOSE_SHAPES)
def test_transpose_host_exact(eng, m, n, fp32):
    a = AC.transpose_input(m, n, fp32)
    out = sentinel_vector(m * n + AC.TAIL, a.dtype.type)
    rc = E.lib().mx_transpose(eng._ctx, fp32, m, n, _vp(a), _vp(out))
    assert rc == 0
    _assert_bits(out, with_tail(_transposed(a)))


@FP
@pytest.mark.parametrize("m,n", AC.TRANSPOSE_SHAPES)
def test_transpose_device_exact(eng, m, n, fp32):
    a = AC.transpose_input(m, n, fp32)
    with Bufs(eng) as bufs:
        din = bufs.put(with_tail(a))
        dout = bufs.put(sentinel_vector(m * n + AC.TAIL, a.dtype.type))
        rc = E.lib().mx_transpose_device(eng._ctx, fp32, m, n, din, dout)
        assert rc == 0
        # the payloads arrive intact, the tail behind n * m is not written
        _assert_bits(bufs.get(dout), with_tail(_transposed(a)))
        _assert_bits(bufs.get(din), with_tail(a))


# ---------------------------------------------------------------------------
# fill_random
@FP
@pytest.mark.parametrize("seed", AC.FILL_SEEDS, ids=hex)
@pytest.mark.parametrize("n", AC.FILL_NS)
def test_fill_random_exact(eng, n, seed, fp32):
    dt = dtype_of(fp32)
    want = sentinel_vector(n + AC.TAIL, dt)
    want[:n] = AC.fill_expected(n, seed, fp32)
    with Bufs(eng) as bufs:
        d = bufs.put(sentinel_vector(n + AC.TAIL, dt))
        eng.fill_random(d, n, seed, fp32=bool(fp32))
        _assert_bits(bufs.get(d), want)


# ---------------------------------------------------------------------------
# zero_pad
@FP
@pytest.mark.parametrize("case", AC.ZERO_PAD_CASES,
                         ids=lambda c: "x".join(map(str, c)))
def test_zero_pad_exact(eng, case, fp32):
    rows_total, cols_total, ld, m, n = case
    img, want = AC.zero_pad_images(case, fp32)
    with Bufs(eng) as bufs:
        d = bufs.put(img)
        eng.zero_pad(d, rows_total, cols_total, ld, m, n, fp32=bool(fp32))
        _assert_bits(bufs.get(d), want)


# ---------------------------------------------------------------------------
# map on special values
def _run_map(eng, op, fp32, a, b, s):
    out = sentinel_vector(a.size + AC.TAIL, a.dtype.type)
    rc = E.lib().mx_map(eng._ctx, Engine.OPS[op], fp32, a.size, _vp(a),
                        _vp(b) if b is not None else None, float(s), _vp(out))
    assert rc == 0
    # the entry writes a.size elements and no more
    _assert_bits(out[a.size:], sentinel_vector(AC.TAIL, a.dtype.type))
    return out[:a.size]


def _assert_map(got, want, keep):
    np.testing.assert_array_equal(np.isnan(got)[keep], np.isnan(want)[keep])
    live = keep & ~np.isnan(want)
    np.testing.assert_array_equal(bits(got)[live], bits(want)[live])


@FP
@pytest.mark.parametrize("op", ["add", "sub", "emul"])
def test_map_binary_specials(eng, op, fp32):
    a, b = AC.map_inputs(fp32)
    want = AC.map_expected(op, a, b, None)
    got = _run_map(eng, op, fp32, a, b, 0.0)
    _assert_map(got, want, np.ones(a.size, dtype=bool))


@FP
@pytest.mark.parametrize("sname", AC.MAP_SCALARS)
@pytest.mark.parametrize("op", ["adds", "subs", "rsubs", "muls"])
def test_map_scalar_specials(eng, op, sname, fp32):
    a, _ = AC.map_inputs(fp32)
    s = AC.map_scalar(sname, fp32)
    want = AC.map_expected(op, a, None, s)
    got = _run_map(eng, op, fp32, a, None, s)
    _assert_map(got, want, np.ones(a.size, dtype=bool))


@FP
@pytest.mark.parametrize("sname", AC.MAP_SCALARS)
@pytest.mark.parametrize("op", ["divs", "rdivs"])
def test_map_division_specials(eng, op, sname, fp32):
    # Lanes whose operand or numpy quotient is subnormal are left out:
    # division of and into subnormals depends on how the compiler expands
    # the divide (fp32 above all), and this project has made no claim about
    # it. Which lanes those are is fixed by the input vector: a quotient is
    # subnormal only where the lane holds the subnormal, the smallest
    # normal or the largest finite value, eight lanes each.
    a, _ = AC.map_inputs(fp32)
    s = AC.map_scalar(sname, fp32)
    want = AC.map_expected(op, a, None, s)
    keep = ~(AC.is_subnormal(a) | AC.is_subnormal(want))
    assert a.size - np.count_nonzero(keep) <= 24
    assert not AC.is_subnormal(np.asarray(s))
    got = _run_map(eng, op, fp32, a, None, s)
    _assert_map(got, want, keep)


# ---------------------------------------------------------------------------
# refusals: one call per guard that oversteps by the least the contract
# refuses (a missing guard would write at most one element past an
# allocation), on sentinel-filled buffers. The restatement of
# _aux_cases.py says of each that it is refused and that its neighbour
# inside the contract is accepted.
def test_aux_refusals_touch_nothing(eng):
    lib, ctx = E.lib(), eng._ctx
    f64, f32 = np.float64, np.float32
    with Bufs(eng) as bufs:
        # mx_fill_random: one element past the end, both types; n < 0
        d100 = bufs.put(sentinel_vector(100, f64))
        assert AC.fill_ok(800, 0, 100) and not AC.fill_ok(800, 0, 101)
        assert lib.mx_fill_random(ctx, d100, 101, 7, 0) == EINVAL
        assert AC.fill_ok(800, 1, 200) and not AC.fill_ok(800, 1, 201)
        assert lib.mx_fill_random(ctx, d100, 201, 7, 1) == EINVAL
        assert lib.mx_fill_random(ctx, d100, -1, 7, 0) == EINVAL

        # mx_zero_pad: image one element longer than the buffer; m past
        # rows_total; n past cols_total; ld short of rows_total
        d23 = bufs.put(sentinel_vector(2 * 8 + 8 - 1, f64))
        assert AC.zero_pad_ok(23 * 8, 0, 7, 3, 8, 4, 2)
        assert not AC.zero_pad_ok(23 * 8, 0, 8, 3, 8, 4, 2)
        assert lib.mx_zero_pad(ctx, d23, 8, 3, 8, 4, 2, 0) == EINVAL
        assert not AC.zero_pad_ok(800, 0, 8, 3, 8, 9, 2)
        assert lib.mx_zero_pad(ctx, d100, 8, 3, 8, 9, 2, 0) == EINVAL
        assert not AC.zero_pad_ok(800, 0, 8, 3, 8, 4, 4)
        assert lib.mx_zero_pad(ctx, d100, 8, 3, 8, 4, 4, 0) == EINVAL
        assert AC.zero_pad_ok(800, 0, 8, 3, 8, 4, 2)
        assert not AC.zero_pad_ok(800, 0, 8, 3, 7, 4, 2)
        assert lib.mx_zero_pad(ctx, d100, 8, 3, 7, 4, 2, 0) == EINVAL
        assert lib.mx_zero_pad(ctx, d100, 8, 3, 8, -1, 2, 0) == EINVAL

        # mx_transpose_device: out one element short; in one element short;
        # in place, by handle; a negative dimension
        d9 = bufs.put(sentinel_vector(9, f64))
        d8 = bufs.put(sentinel_vector(8, f64))
        assert AC.transpose_ok(0, 3, 3, 72, 72)
        assert not AC.transpose_ok(0, 3, 3, 72, 64)
        assert lib.mx_transpose_device(ctx, 0, 3, 3, d9, d8) == EINVAL
        assert lib.mx_transpose_device(ctx, 0, 3, 3, d8, d9) == EINVAL
        assert lib.mx_transpose_device(ctx, 0, 3, 3, d9, d9) == EINVAL
        assert lib.mx_transpose_device(ctx, 0, -1, 3, d9, d100) == EINVAL
        assert lib.mx_transpose_device(ctx, 1, 3, 6, d9, d8) == EINVAL

        # mx_dgemv_device: lda = m - 1; image one element past dA
        x = np.ones(3)
        y = sentinel_vector(8, f64)
        xp = x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        yp = y.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        assert AC.gemv_ok(800, 8, 3, 8) and not AC.gemv_ok(800, 8, 3, 7)
        assert lib.mx_dgemv_device(ctx, 8, 3, d100, 7, xp, yp) == EINVAL
        assert AC.gemv_ok(23 * 8, 7, 3, 8)
        assert not AC.gemv_ok(23 * 8, 8, 3, 8)
        assert lib.mx_dgemv_device(ctx, 8, 3, d23, 8, xp, yp) == EINVAL
        _assert_bits(y, sentinel_vector(8, f64))

        # pitched transfers: pitch = m - 1; one element past; a bad elem
        host = sentinel_vector(64, f64)
        keep = host.copy()
        src = np.ones(64)
        assert AC.copy2d_ok(800, 8, 0, 8, 8, 3)
        assert not AC.copy2d_ok(800, 8, 0, 7, 8, 3)
        assert not AC.copy2d_ok(23 * 8, 8, 0, 8, 8, 3)
        assert AC.copy2d_ok(23 * 8, 8, 0, 8, 7, 3)
        assert not AC.copy2d_ok(800, 2, 0, 8, 8, 3)
        assert AC.copy2d_ok(24 * 8, 8, 0, 8, 8, 3)
        assert not AC.copy2d_ok(24 * 8, 8, 8, 8, 8, 3)
        d24 = bufs.put(sentinel_vector(24, f64))
        assert lib.mx_download2d(ctx, _vp(host), d100, 7, 8, 3, 8) == EINVAL
        assert lib.mx_download2d(ctx, _vp(host), d23, 8, 8, 3, 8) == EINVAL
        assert lib.mx_download2d(ctx, _vp(host), d100, 8, 8, 3, 2) == EINVAL
        assert lib.mx_download2d_off(ctx, _vp(host), d100, 0, 7, 8, 3,
                                     8) == EINVAL
        assert lib.mx_download2d_off(ctx, _vp(host), d24, 8, 8, 8, 3,
                                     8) == EINVAL
        assert lib.mx_download2d_off(ctx, _vp(host), d24, -8, 8, 8, 3,
                                     8) == EINVAL
        assert lib.mx_upload2d(ctx, d100, 7, _vp(src), 8, 3, 8) == EINVAL
        assert lib.mx_upload2d(ctx, d23, 8, _vp(src), 8, 3, 8) == EINVAL
        assert lib.mx_upload2d(ctx, d100, 8, _vp(src), 8, 3, 2) == EINVAL
        _assert_bits(host, keep)

        # whole-buffer transfers and memset: a negative size, one byte past
        assert not AC.bytes_ok(800, -1) and not AC.bytes_ok(800, 801)
        assert lib.mx_download(ctx, _vp(host), d100, -1) == EINVAL
        assert lib.mx_download(ctx, _vp(host), d8, 65) == EINVAL
        assert lib.mx_memset(ctx, d100, -1) == EINVAL
        assert lib.mx_memset(ctx, d100, 801) == EINVAL
        assert lib.mx_upload(ctx, d100, _vp(src), -1) == EINVAL
        _assert_bits(host, keep)

        # mx_map: op = 9 and op = -1 (neither runs as RDIVS or as binary)
        a = np.ones(8)
        out = sentinel_vector(8, f64)
        assert not AC.map_op_ok(9) and not AC.map_op_ok(-1)
        assert AC.map_op_ok(8) and AC.map_op_ok(0)
        assert lib.mx_map(ctx, 9, 0, 8, _vp(a), None, 2.0, _vp(out)) == EINVAL
        assert lib.mx_map(ctx, -1, 0, 8, _vp(a), _vp(a), 2.0,
                          _vp(out)) == EINVAL
        _assert_bits(out, sentinel_vector(8, f64))

        bufs.assert_untouched()

        # fp32 handles share the checks: one element past, in elements of 4
        d50 = bufs.put(sentinel_vector(50, f32))
        assert lib.mx_fill_random(ctx, d50, 51, 7, 1) == EINVAL
        assert AC.zero_pad_ok(200, 1, 2, 7, 8, 2, 2)
        assert not AC.zero_pad_ok(200, 1, 3, 7, 8, 2, 2)
        assert lib.mx_zero_pad(ctx, d50, 3, 7, 8, 2, 2, 1) == EINVAL
        bufs.assert_untouched()


def test_aux_noops_touch_nothing(eng):
    lib, ctx = E.lib(), eng._ctx
    with Bufs(eng) as bufs:
        d = bufs.put(sentinel_vector(100, np.float64))
        d2 = bufs.put(sentinel_vector(100, np.float64))
        assert lib.mx_fill_random(ctx, d, 0, 7, 0) == 0
        assert lib.mx_transpose_device(ctx, 0, 0, 5, d, d2) == 0
        assert lib.mx_transpose_device(ctx, 0, 5, 0, d, d2) == 0
        assert lib.mx_transpose_device(ctx, 1, 0, 0, d, d2) == 0
        assert lib.mx_zero_pad(ctx, d, 0, 5, 8, 0, 3, 0) == 0
        assert lib.mx_zero_pad(ctx, d, 8, 0, 8, 4, 0, 0) == 0
        assert lib.mx_zero_pad(ctx, d, 0, 0, 0, 0, 0, 1) == 0
        assert lib.mx_memset(ctx, d, 0) == 0
        bufs.assert_untouched()
        # the engine still serves: a real call after the refused ones
        assert lib.mx_fill_random(ctx, d, 100, 0xA11CE, 0) == 0
        _assert_bits(bufs.get(d), AC.fill_expected(100, 0xA11CE, 0))
