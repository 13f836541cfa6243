"""IEEE 754 binary64 division, multiplication, addition, square root and the reference's normalisation (TRT.c:439-450), correctly
rounded to nearest even by Python integers and fractions alone: a judge that shares no floating-point unit with what it judges.

A double enters and leaves as its 64-bit pattern (struct / numpy views: no arithmetic).  Everything that decides a bit is integer
arithmetic; nothing here adds, multiplies, divides, compares or takes the root of a float."""
import math
import struct
from fractions import Fraction

import numpy as np

SIGN = 1 << 63
EXP_MASK = 0x7FF << 52
FRAC_MASK = (1 << 52) - 1
INF = EXP_MASK
NAN = EXP_MASK | (1 << 51)
HIDDEN = 1 << 52
TEN_THOUSANDTH = 0x3F1A36E2EB1C432D  # the double 0.0001 of TRT.c:444


def to_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


assert to_bits(float.fromhex("0x1.a36e2eb1c432dp-14")) == TEN_THOUSANDTH and repr(from_bits(TEN_THOUSANDTH)) == "0.0001"


def is_nan(b):
    return (b & ~SIGN) > INF


def is_inf(b):
    return (b & ~SIGN) == INF


def is_zero(b):
    return (b & ~SIGN) == 0


def decode(b):
    """(m, e) with |value| = m * 2^e, m an integer below 2^53; finite patterns only"""
    exp, frac = (b & EXP_MASK) >> 52, b & FRAC_MASK
    return (frac, -1074) if exp == 0 else (frac | HIDDEN, exp - 1075)


def round_ratio(n, d):
    """The pattern (sign clear) of n / d, integers n > 0 and d > 0, rounded to nearest even: normals, denormals (one rounding at
    the denormal's own precision), and infinity from 2^1024 - 2^970 upwards."""
    e = n.bit_length() - d.bit_length()  # 2^(e-1) < n/d < 2^(e+1)
    if (n >= d << e) if e >= 0 else (n << -e >= d):
        top = e                          # 2^top <= n/d < 2^(top+1)
    else:
        top = e - 1
    q = max(top, -1022) - 52             # the exponent of the last place kept
    if q >= 0:
        k, rem = divmod(n, d << q)
        den = d << q
    else:
        k, rem = divmod(n << -q, d)
        den = d
    if 2 * rem > den or (2 * rem == den and k & 1):
        k += 1
    # k < 2^52 at q = -1074 is a denormal, whose pattern is k itself; 2^52 <= k < 2^53 adds its hidden bit to the exponent field,
    # and a k that the rounding carried to 2^53 (or a denormal's to 2^52) steps the exponent by the same addition
    b = ((q + 1074) << 52) + k
    return b if b < INF else INF


def rn(value, zero_sign=0):
    """Fraction -> float, rounded to nearest even; the caller supplies the sign of an exact zero (0 or 1)"""
    value = Fraction(value)
    if value == 0:
        return from_bits(SIGN if zero_sign else 0)
    return from_bits((SIGN if value < 0 else 0) | round_ratio(abs(value.numerator), value.denominator))


def div_bits(a, b):
    sign = (a ^ b) & SIGN
    if is_nan(a) or is_nan(b):
        return NAN
    if is_inf(a):
        return NAN if is_inf(b) else sign | INF
    if is_inf(b):
        return sign
    if is_zero(b):
        return NAN if is_zero(a) else sign | INF
    if is_zero(a):
        return sign
    (ma, ea), (mb, eb) = decode(a), decode(b)
    e = ea - eb
    return sign | (round_ratio(ma << e, mb) if e >= 0 else round_ratio(ma, mb << -e))


def mul_bits(a, b):
    sign = (a ^ b) & SIGN
    if is_nan(a) or is_nan(b):
        return NAN
    if is_inf(a) or is_inf(b):
        return NAN if is_zero(a) or is_zero(b) else sign | INF
    if is_zero(a) or is_zero(b):
        return sign
    (ma, ea), (mb, eb) = decode(a), decode(b)
    e = ea + eb
    return sign | (round_ratio(ma * mb << e, 1) if e >= 0 else round_ratio(ma * mb, 1 << -e))


def add_bits(a, b):
    if is_nan(a) or is_nan(b):
        return NAN
    if is_inf(a):
        return NAN if is_inf(b) and (a ^ b) & SIGN else a
    if is_inf(b):
        return b
    (ma, ea), (mb, eb) = decode(a), decode(b)
    e = min(ea, eb)
    total = (-(ma << ea - e) if a & SIGN else ma << ea - e) + (-(mb << eb - e) if b & SIGN else mb << eb - e)
    if total == 0:
        return a & b & SIGN  # -0 only from (-0) + (-0); x + (-x) is +0 in round to nearest
    sign = SIGN if total < 0 else 0
    return sign | (round_ratio(abs(total) << e, 1) if e >= 0 else round_ratio(abs(total), 1 << -e))


def sqrt_bits(x):
    if is_nan(x):
        return NAN
    if is_zero(x):
        return x
    if x & SIGN:
        return NAN
    if is_inf(x):
        return x
    m, e = decode(x)
    shift = 116 + (e & 1)                # e - shift even, and the integer root below has at least 58 bits
    scaled = m << shift
    root = math.isqrt(scaled)            # root <= sqrt(scaled) < root + 1
    exact = root * root == scaled
    # With 58 bits or more, every double and every midpoint between two doubles in [root, root + 1] is an integer, so sqrt(scaled)
    # strictly between root and root + 1 rounds as root + 1/2 does.  A tie would need an exact root of 54 significant bits, whose
    # square has more than 53: impossible for a double.  An exact root (the radicand a perfect square) has at most 27.
    n = 2 * root + (0 if exact else 1)
    h = (e - shift) // 2 - 1             # the root is n * 2^h
    out = round_ratio(n << h, 1) if h >= 0 else round_ratio(n, 1 << -h)
    if exact:
        mr, er = decode(out)
        assert mr * mr * Fraction(2) ** (2 * er) == m * Fraction(2) ** e, "an exact root is representable"
    return out


def greater_bits(a, b):
    """a > b as IEEE compares them (false with a NaN; -0 equals +0)"""
    if is_nan(a) or is_nan(b):
        return False
    key = lambda v: -(v & ~SIGN) if v & SIGN else v
    return key(a) > key(b)


def unit_bits(x, y, z):
    """TRT.c:439-450: length = sqrt((x*x + y*y) + z*z), every product and sum rounded; three divisions when length > 0.0001,
    the vector's own bits otherwise.  Returns (x', y', z', length)."""
    length = sqrt_bits(add_bits(add_bits(mul_bits(x, x), mul_bits(y, y)), mul_bits(z, z)))
    if greater_bits(length, TEN_THOUSANDTH):
        return div_bits(x, length), div_bits(y, length), div_bits(z, length), length
    return x, y, z, length


def div(a, b):
    return from_bits(div_bits(to_bits(a), to_bits(b)))


def mul(a, b):
    return from_bits(mul_bits(to_bits(a), to_bits(b)))


def add(a, b):
    return from_bits(add_bits(to_bits(a), to_bits(b)))


def sqrt(x):
    return from_bits(sqrt_bits(to_bits(x)))


def unit(x, y, z):
    return tuple(from_bits(v) for v in unit_bits(to_bits(x), to_bits(y), to_bits(z))[:3])


# ---- whole arrays -------------------------------------------------------------------------------------------------------------

def patterns(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel().tolist()


def doubles(bit_list, shape=None):
    out = np.array(bit_list, dtype=np.uint64).view(np.float64)
    return out if shape is None else out.reshape(shape)


def div_array(a, b):
    return doubles([div_bits(p, q) for p, q in zip(patterns(a), patterns(b))])


def sqrt_array(x):
    return doubles([sqrt_bits(p) for p in patterns(x)])


def unit_array(xyz):
    """[n, 3] vectors -> ([n, 3] normalised, [n] lengths)"""
    p = patterns(xyz)
    out = [unit_bits(p[i], p[i + 1], p[i + 2]) for i in range(0, len(p), 3)]
    return doubles([v for rec in out for v in rec[:3]], (-1, 3)), doubles([rec[3] for rec in out])


def same_bits(got, want):
    """elementwise: the same pattern, or NaN with NaN (any payload)"""
    g, w = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    return (g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))
