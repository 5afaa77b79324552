# An exact fused multiply-add in numpy: fma(x, y, z) = round(x * y + z), one
# rounding, elementwise, for float32 and float64 arrays. The restatements of
# the diagonal kernels (_getrf_cases.eliminate_restated,
# _trsm_cases.substitute_restated) are built on it, so that a GPU test can
# state a kernel's bits without a compiler. test_diag_bits_cpu.py proves it
# against the compiler's own fma on several hundred thousand triples.
#
# fp32. The product of two float32 is exact in float64 (48 bits of 53, and
#   its exponent lies within float64's range whatever the operands). TwoSum
#   with the addend gives the float64 sum s and its exact error e. s is then
#   ROUNDED TO ODD: where e != 0 and s's last mantissa bit is even, s moves
#   one ulp toward e, so that s is the truncated exact sum with its last bit
#   set whenever anything was lost (had s been rounded up, the step down is
#   the truncation). A value rounded to odd at 53 bits rounds to the same
#   float32 as the exact value, because 53 >= 24 + 2 (Boldo, Melquiond:
#   "Emulation of FMA and correctly rounded sums", 2008). That holds over the
#   whole range: float32's subnormals are 2^-149 multiples, normal numbers of
#   float64, and astype(float32) rounds into them correctly.
#
# fp64. Veltkamp's split and Dekker's product give x * y = uh + ul exactly;
#   (th, tl) = TwoSum(z, uh); v = RoundToOdd(tl + ul); the result is th + v
#   (Boldo, Melquiond, Algorithm 5 "Fma emulation"). It is valid only where
#   nothing underflows or overflows on the way:
#       2^-400 <= |x|, |y| <= 2^400, and z = 0 or 2^-900 <= |z| <= 2^900,
#   (the split multiplies by 2^27 + 1; ul, of magnitude |x y| 2^-53 or
#   less, must stay a normal number for the product to be exact). in_range64
#   states it and the callers keep their fp64 data inside it; zeros pass.
#
# Infinities and NaN: a non-finite operand is given the plain x * y + z,
# whose class (inf of a sign, or NaN) is the fused one's, the intermediate
# TwoSum would turn an infinity into a NaN.
import numpy as np


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_to_odd(s, e):
    """s, e float64 with s + e exact and s = fl(s + e): the sum rounded to
    odd."""
    bits = s.view(np.int64)
    even = (bits & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    # toward e: away from zero (bits + 1) where e has s's sign. s = 0 with
    # e != 0 cannot occur (s is the rounded sum, e below half its ulp).
    away = (e > 0) == (s > 0)
    out = np.where(fix, bits + np.where(away, 1, -1), bits)
    return out.view(np.float64)


def fma32(x, y, z):
    x, y, z = (np.asarray(v, dtype=np.float32) for v in (x, y, z))
    with np.errstate(all="ignore"):
        p = x.astype(np.float64) * y.astype(np.float64)
        zd = z.astype(np.float64)
        p, zd = np.broadcast_arrays(p, zd)
        s, e = _two_sum(p, zd)
        r = _round_to_odd(np.ascontiguousarray(s), e).astype(np.float32)
        plain = (p + zd).astype(np.float32)
    return np.where(np.isfinite(p) & np.isfinite(zd), r, plain)


_SPLIT = np.float64(2.0 ** 27 + 1)


def _split(a):
    c = _SPLIT * a
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def in_range64(*arrays, addend=None):
    """True where fma64 is valid: every factor zero or in [2^-400, 2^400],
    the addend zero or in [2^-900, 2^900]."""
    ok = True
    for a in arrays:
        m = np.abs(np.asarray(a, dtype=np.float64))
        ok = ok and bool(np.all((m == 0) | ((m >= 2.0 ** -400) &
                                            (m <= 2.0 ** 400))))
    if addend is not None:
        m = np.abs(np.asarray(addend, dtype=np.float64))
        ok = ok and bool(np.all((m == 0) | ((m >= 2.0 ** -900) &
                                            (m <= 2.0 ** 900))))
    return ok


def fma64(x, y, z):
    x, y, z = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64)
                                    for v in (x, y, z)))
    with np.errstate(all="ignore"):
        uh, ul = _two_prod(x, y)
        th, tl = _two_sum(z, uh)
        w, we = _two_sum(tl, ul)
        r = th + _round_to_odd(np.ascontiguousarray(w), we)
        plain = x * y + z
    return np.where(np.isfinite(x) & np.isfinite(y) & np.isfinite(z), r,
                    plain)


def fma(x, y, z):
    """Elementwise fma in the operands' common type, float32 or float64."""
    dt = np.result_type(x, y, z)
    if dt == np.float32:
        return fma32(x, y, z)
    assert dt == np.float64, dt
    return fma64(x, y, z)
