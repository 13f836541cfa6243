"""The specular term of ONE light at ONE hit, written from the declared rules above trt_set_specular in include/trt_hip.h -- not from
the kernels and not from tests/specular_restatement.c.

Every operation of the term is a correctly rounded binary64 multiplication, addition, division or square root, or the reference's
normalisation: those of tests/exact_ieee.py, which works on bit patterns with Python integers and shares no floating-point unit with
what it judges.  So the model predicts spec bit for bit from the doubles that enter the term; nothing accumulates along a path.

    view  = -d
    half  = normalize_vector(light_direction + view)        a vector no longer than 1e-4 is left alone
    c     = clamp(dot(normal, half), 0.0, 1.0)              a NaN passes through
    s     = powi(c, n)                                      n from the specularity: 0 unless e >= 0, 65535 from there up, else truncated
    spec  = light.color * s                                 directional light
    spec  = light.color * (light_intensity * s)             point light
"""
from fractions import Fraction

import exact_ieee as X

ZERO, ONE, SIGN = X.to_bits(0.0), X.to_bits(1.0), X.SIGN
TOP = X.to_bits(65535.0)


def exponent_of(e):
    """n of a specularity given as its pattern"""
    if X.is_nan(e) or X.greater_bits(ZERO, e):  # !(e >= 0)
        return 0
    if not X.greater_bits(TOP, e):  # e >= 65535, infinity too
        return 65535
    m, x = X.decode(e)
    return m << x if x >= 0 else m >> -x  # truncated


def powi(c, n):
    """binary exponentiation, right to left, each product one rounded multiplication; patterns in, pattern out"""
    r, b = ONE, c
    while n:
        if n & 1:
            r = X.mul_bits(r, b)
        n >>= 1
        if n:
            b = X.mul_bits(b, b)
    return r


def clamp01(v):
    if X.greater_bits(ZERO, v):
        return ZERO
    if X.greater_bits(v, ONE):
        return ONE
    return v  # a NaN, and -0.0, pass through


def dot(a, b):
    return X.add_bits(X.add_bits(X.mul_bits(a[0], b[0]), X.mul_bits(a[1], b[1])), X.mul_bits(a[2], b[2]))


def term(d, normal, light_direction, light_intensity, colour, e, point_light, normalise=True):
    """patterns in (d, normal, light_direction, colour: three each); returns (spec: three patterns, what was met on the way: the
    length of light_direction + view and dot(normal, half) before the clamp, as patterns).  normalise=False is a planted mistake."""
    view = [v ^ SIGN for v in d]  # -d: the sign alone changes, of a NaN too
    summed = [X.add_bits(l, v) for l, v in zip(light_direction, view)]
    hx, hy, hz, length = X.unit_bits(*summed)
    half = [hx, hy, hz] if normalise else summed
    raw = dot(normal, half)
    s = powi(clamp01(raw), exponent_of(e))
    by = X.mul_bits(light_intensity, s) if point_light else s
    return [X.mul_bits(c, by) for c in colour], {"half_length": length, "dot": raw}


def exact_power(c, n):
    """c^n as a rational, for a finite double c"""
    m, x = X.decode(X.to_bits(c))
    return (Fraction(m) * Fraction(2) ** x) ** n
