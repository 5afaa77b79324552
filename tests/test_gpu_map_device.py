# mx_map_device (Engine.map_raw): the elementwise kernel of mx_map on device
# buffers. Exact small-integer data for every op, out of place and in both
# documented in-place forms (dC = dA, dC = dB), with a NaN sentinel behind
# the n elements that must survive; refusals and the empty call touch
# nothing.
import numpy as np
import pytest

from _exact import UINT, _dev, _filled, _nan, dtype_of
from marlin_amd import Engine

pytestmark = pytest.mark.gpu

EINVAL = -4
N, TAIL = 1000, 24          # odd-ish length: the grid-stride loop's last lap

# name -> numpy restatement; operands are chosen so each result is exact
OPS = {
    "add": lambda a, b, s: a + b, "sub": lambda a, b, s: a - b,
    "emul": lambda a, b, s: a * b, "adds": lambda a, b, s: a + s,
    "subs": lambda a, b, s: a - s, "rsubs": lambda a, b, s: s - a,
    "muls": lambda a, b, s: a * s, "divs": lambda a, b, s: a / s,
    "rdivs": lambda a, b, s: s / a,
}
BINARY = ("add", "sub", "emul")


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _operands(dt):
    rng = np.random.RandomState(5)
    a = rng.randint(-64, 65, size=N).astype(dt)
    b = rng.randint(-64, 65, size=N).astype(dt)
    a[a == 0] = 3                            # rdivs divides by a
    return a, b


def _with_tail(v, dt):
    img = _filled(N + TAIL, 1, _nan(dt))[:, 0].copy()
    img[:N] = v
    return img


def _fetch(eng, d, like):
    got = np.empty_like(like)
    eng.download(got, d, got.nbytes)
    return got


# every op out of place and over dA; the binary ones over dB too
FORMS = [(op, where) for op in OPS for where in ("out", "dC=dA", "dC=dB")
         if where != "dC=dB" or op in BINARY]


@pytest.mark.parametrize("op,where", FORMS, ids=[f"{o}-{w}" for o, w in FORMS])
@pytest.mark.parametrize("fp32", [0, 1], ids=["f64", "f32"])
def test_map_device_exact(eng, fp32, op, where):
    dt = dtype_of(fp32)
    U = UINT[dt]
    a, b = _operands(dt)
    s = dt(-4)                               # a power of two: divs is exact
    if op == "rdivs":
        a = np.where(a % 2 == 0, dt(2), dt(-8)).astype(dt)   # s / a exact
    want = OPS[op](a, b, s).astype(dt)
    aimg, bimg = _with_tail(a, dt), _with_tail(b, dt)
    cimg = _filled(N + TAIL, 1, _nan(dt))[:, 0].copy()
    bufs = []
    try:
        dA, dB = _dev(eng, aimg, bufs), _dev(eng, bimg, bufs)
        dC = {"out": None, "dC=dA": dA, "dC=dB": dB}[where] or _dev(
            eng, cimg, bufs)
        assert eng.map_raw(op, N, dA, dB if op in BINARY else None, float(s),
                           dC, bool(fp32), check=False) == 0
        got = _fetch(eng, dC, cimg)
        np.testing.assert_array_equal(got[:N].view(U), want.view(U))
        # the tail behind the n elements is not written, operands not named
        # as dC are not touched
        assert (got[N:].view(U) == _nan(dt).view(U)).all()
        if where != "dC=dA":
            np.testing.assert_array_equal(_fetch(eng, dA, aimg).view(U),
                                          aimg.view(U))
        if where != "dC=dB":
            np.testing.assert_array_equal(_fetch(eng, dB, bimg).view(U),
                                          bimg.view(U))
    finally:
        for d in bufs:
            eng.free(d)


def test_map_device_refusals_touch_nothing(eng):
    from marlin_amd import engine as E
    dt, U = np.float64, np.uint64
    img = _filled(N, 1, _nan(dt))[:, 0].copy()
    short = _filled(N - 1, 1, _nan(dt))[:, 0].copy()
    bufs = []
    try:
        dA, dB, dC = (_dev(eng, img, bufs) for _ in range(3))
        dS = _dev(eng, short, bufs)

        def call(op=E.Engine.OPS["add"], fp32=0, n=N, A=dA, B=dB, C=dC):
            return E.lib().mx_map_device(eng._ctx, op, fp32, n, A, B, 2.0, C)
        refused = {
            "op = -1": dict(op=-1), "op = 9": dict(op=9),
            "is_fp32 = 2": dict(fp32=2), "n = -1": dict(n=-1),
            "n one past every buffer": dict(n=N + 1),
            "dA one element short": dict(A=dS),
            "dB one element short": dict(B=dS),
            "dC one element short": dict(C=dS),
            "binary op without dB": dict(B=None),
            "dA NULL": dict(A=None), "dC NULL": dict(C=None),
        }
        for what, kw in refused.items():
            assert call(**kw) == EINVAL, what
        # fp32 halves the bytes: twice the elements fit, one more does not
        assert call(fp32=1, n=2 * N + 1) == EINVAL
        # a scalar op does not look at dB; the empty call is a no-op
        assert call(op=E.Engine.OPS["muls"], B=None, n=0) == 0
        assert call(n=0) == 0
        for d, like in ((dA, img), (dB, img), (dC, img), (dS, short)):
            np.testing.assert_array_equal(_fetch(eng, d, like).view(U),
                                          like.view(U))
        # the calls they neighbour pass
        assert call(op=E.Engine.OPS["muls"], B=None, A=dS, C=dS, n=N - 1) == 0
        assert call(fp32=1, n=2 * N) == 0
    finally:
        for d in bufs:
            eng.free(d)
