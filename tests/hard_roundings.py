"""Operands whose exact quotient or root lies next to a rounding boundary, and vectors steered so that their computed length is
such a divisor: the inputs that tell "correctly rounded" from "nearly" (tests/test_hard_roundings.py; the judge is tests/exact_ieee.py).

Every family is seeded, built once per process, and returned as float64 arrays (treat them as read-only).  The constructions are
number theory on the significands; a power of two places them in the range.  What each family claims about itself is verified by
integer arithmetic in the CPU tests."""
import functools
import math
import random

import numpy as np

MIDPOINT_CLAIM_DIV = 49   # (a): within 2^-49 ulp of a midpoint of the result's precision
MIDPOINT_CLAIM_SQRT = 30  # (c), (d): within 2^-30 ulp
WAVE = 64


def _f(m, e):
    """m * 2^e, exactly (the callers choose m and e so that it is a double)"""
    return math.ldexp(float(m), e)


def _signed(rng, v):
    return -v if rng.getrandbits(1) else v


# ---- (a) division: a worst case at every result precision -----------------------------------------------------------------------

def division_pair(rng, p, bbits=53, rmax=15, amax=None):
    """(A, B): B odd with exactly `bbits` bits, and A / B = M / 2^(p+1) - r / (2^(p+1) B) for an odd M of p + 1 bits and an odd
    |r| <= rmax: the quotient, in [1/2, 1), is |r| / (2 B) ulp (of p bits) from the midpoint M / 2^(p+1); r < 0 above it, r > 0 below."""
    mod = 1 << (p + 1)
    while True:
        B = (rng.getrandbits(bbits - 2) << 1 | 1) + (1 << (bbits - 1))
        r = _signed(rng, rng.randrange(1, rmax + 1, 2))
        M = r * pow(B, -1, mod) % mod
        if M < 1 << p:
            continue
        A = (B * M - r) >> (p + 1)
        if amax is None or A < amax:
            return A, B


@functools.lru_cache(maxsize=None)
def division_hard():
    """dict a, b, p (the significant bits of the correctly rounded quotient: 53, or fewer for a denormal one), kind"""
    rng = random.Random(0xD1F)
    a, b, p, kind = [], [], [], []

    def emit(A, ea, B, eb, bits, name):
        a.append(_signed(rng, _f(A, ea))), b.append(_signed(rng, _f(B, eb))), p.append(bits), kind.append(name)

    for _ in range(20000):  # anywhere in the middle of the range
        A, B = division_pair(rng, 53)
        eb = rng.randrange(-353, 247)
        emit(A, eb + rng.randrange(-100, 101), B, eb, 53, "mid")
    for _ in range(2000):   # the quotient in [2^1023, 2^1024): the last binade below overflow
        A, B = division_pair(rng, 53)
        emit(A, 460, B, -564, 53, "top_binade")
    for _ in range(1000):   # ... and past it: infinity
        A, B = division_pair(rng, 53)
        emit(A, 460, B, -565 - rng.randrange(0, 40), 53, "overflow")
    for bits in range(1, 53):  # a denormal quotient of exactly `bits` significant bits: ONE rounding, at that precision
        for _ in range(1200 if bits in (52, 40, 20, 5, 1) else 150):
            A, B = division_pair(rng, bits)
            emit(A, -553, B, 521 - bits, bits, "denormal_quotient")
    for _ in range(1500):   # a denormal numerator: A below 2^52 loses no bit
        A, B = division_pair(rng, 53, amax=1 << 52)
        emit(A, -1074, B, rng.choice((-1074, -1000, -600)), 53, "denormal_numerator")
    for _ in range(1500):   # a denormal denominator: B of 52 bits, and |r| <= 7 keeps the distance under 2^-49 ulp
        A, B = division_pair(rng, 53, bbits=52, rmax=7)
        emit(A, rng.choice((-1074, -1000, -200)), B, -1074, 53, "denormal_denominator")
    return {"a": np.array(a), "b": np.array(b), "p": np.array(p), "kind": np.array(kind)}


@functools.lru_cache(maxsize=None)
def division_threshold():
    """quotients about DBL_MAX and the overflow threshold 2^1024 - 2^970, and about the smallest normal and denormal: judged, not hard"""
    a, b = [], []
    for i in range(8):
        for j in range(8):
            a.append(_f((1 << 53) - 1 - j, 971)), b.append(_f((1 << 53) - i, -53))   # about 2^1024 from either side
            a.append(_f((1 << 53) - 1 - j, 971)), b.append(_f((1 << 52) + i, -52))
            a.append(_f((1 << 52) + j, -1074)), b.append(_f((1 << 52) + i, -52))     # about 2^-1022
            a.append(_f((1 << 52) + j, -1074)), b.append(_f((1 << 53) - i, -53))
            a.append(_f(1 + j, -1074)), b.append(_f(2 + i, 0))                       # the last denormals, ties to zero and to one
    return {"a": np.array(a), "b": np.array(b)}


# ---- (b) division: exact and nearly exact ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def division_exact():
    rng = random.Random(0xB)
    a, b = [], []
    for _ in range(1500):
        q, d = rng.getrandbits(26) | 1 << 25, rng.getrandbits(26) | 1 << 25
        ea, eb = rng.randrange(-400, 400), rng.randrange(-400, 400)
        prod, div = _signed(rng, _f(q * d, ea)), _signed(rng, _f(d, eb))
        a += [prod, np.nextafter(prod, np.inf), np.nextafter(prod, -np.inf)]         # a = q b, and one ulp either way
        b += [div] * 3
    for _ in range(500):
        v = _signed(rng, _f(rng.getrandbits(53) | 1 << 52, rng.randrange(-1074, 971)))
        a += [v, v]                                                                   # a == b
        b += [v, -v]
    for _ in range(500):                                                              # powers of two, every kind of quotient
        a.append(_signed(rng, _f(1, rng.randrange(-1074, 1024)))), b.append(_signed(rng, _f(1, rng.randrange(-1074, 1024))))
    for _ in range(500):
        a.append(_signed(rng, _f(rng.getrandbits(53) | 1 << 52, rng.randrange(-1074, 971)))), b.append(_f(1, rng.randrange(-1074, 1024)))
    for _ in range(1000):                                                             # denormal operands with random significands
        den = _signed(rng, _f(rng.getrandbits(rng.randrange(1, 53)) | 1, -1074))
        other = _signed(rng, _f(rng.getrandbits(53) | 1 << 52, rng.choice((-1074, -1070, -1000, -53, 900))))
        third = _signed(rng, _f(rng.getrandbits(rng.randrange(1, 53)) | 1, -1074))
        a += [den, other, den]
        b += [other, den, third]
    special = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 5e-324, 1.7976931348623157e308, 2.2250738585072014e-308]
    for s in special:
        for t in special:
            a.append(s), b.append(t)
    return {"a": np.array(a), "b": np.array(b)}


# ---- (c) square root, closed form -----------------------------------------------------------------------------------------------

# 4^j places [1, 4) in the range: the middle; the two binades just inside sqrt_exact's window (2^-300 <= x < 2^300) at either end, the
# two just outside; the ends of the normal range
SQRT_SCALES = {"mid": (0, 7, -33), "inside_low": (-150,), "inside_high": (149,), "outside_low": (-151,), "outside_high": (150,),
               "range_ends": (-511, 510)}


def _root_scales():
    return [(name, j) for name, js in SQRT_SCALES.items() for j in js]


@functools.lru_cache(maxsize=None)
def sqrt_closed_form():
    """1 + m 2^-52 (root just below the midpoint 1 + m 2^-53) and 4 - m 2^-51 (root just below the midpoint 2 - m 2^-53), odd m < 2000,
    times 4^j.  The root of every one lies BELOW its midpoint: sqrt is concave, so no closed form of this kind lies above."""
    x, kind = [], []
    for m in range(1, 2000, 2):
        for name, j in _root_scales():
            x.append(_f((1 << 52) + m, -52 + 2 * j)), kind.append(name)
            x.append(_f((1 << 53) - m, -51 + 2 * j)), kind.append(name)
    return {"x": np.array(x), "kind": np.array(kind)}


# ---- (d) square root, modular ---------------------------------------------------------------------------------------------------

def square_roots_mod(r, k):
    """the four square roots of r modulo 2^k (r = 1 mod 8, k >= 3), lifted bit by bit from the roots modulo 8"""
    s = 1
    for i in range(3, k):                  # s^2 = r (mod 2^i) -> (mod 2^(i+1)): if bit i of s^2 - r is set, adding 2^(i-1) flips it
        if (s * s - r) >> i & 1:
            s += 1 << (i - 1)
    half = 1 << (k - 1)
    roots = sorted({t % (1 << k) for t in (s, -s, s + half, -s + half)})
    assert len(roots) == 4 and all((t * t - r) % (1 << k) == 0 for t in roots)
    return roots


@functools.lru_cache(maxsize=None)
def sqrt_modular_base():
    """(A, k, M, r): A 2^k = M^2 - r, M odd of 54 bits, so that sqrt(A 2^k) is |r| / (4 M) ulp from the midpoint M; r > 0 below it"""
    out = []
    for r in range(-3999, 4000, 8):
        for k in (53, 54, 55):
            for M in square_roots_mod(r, k):
                if not 1 << 53 <= M < 1 << 54:
                    continue
                A = (M * M - r) >> k
                if A.bit_length() <= 53:
                    out.append((A, k, M, r))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sqrt_modular():
    x, kind = [], []
    for A, k, M, r in sqrt_modular_base():
        for name, j in _root_scales():     # A 2^k is in [2^106, 2^108): 4^-53 brings it to [1, 4), 4^j places it
            x.append(_f(A, k - 106 + 2 * j)), kind.append(name)
    return {"x": np.array(x), "kind": np.array(kind)}


@functools.lru_cache(maxsize=None)
def sqrt_exact_and_denormal():
    """perfect squares with their two neighbours, denormal arguments with random significands, and the specials: judged, not hard"""
    rng = random.Random(0x5)
    x = []
    for _ in range(1500):
        n = rng.getrandbits(26) | 1 << 25
        sq = _f(n * n, 2 * rng.choice((0, -26, -150, -151, -176, 124, 125, 480, -520)))
        x += [sq, np.nextafter(sq, np.inf), np.nextafter(sq, 0.0)]
    for _ in range(3000):
        x.append(_f(rng.getrandbits(rng.randrange(1, 53)) | 1, -1074))
    x += [0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -5e-324, 5e-324, 1.7976931348623157e308, 2.2250738585072014e-308,
          2.0 ** -300, np.nextafter(2.0 ** -300, 0.0), 2.0 ** 300, np.nextafter(2.0 ** 300, 0.0)]
    return {"x": np.array(x)}


@functools.lru_cache(maxsize=None)
def sqrt_inside_window():
    """the hard square-root arguments (c) and (d) that lie inside sqrt_exact's window: fourth fields for uniform waves"""
    c, d = sqrt_closed_form(), sqrt_modular()
    inside = lambda f: f["x"][np.isin(f["kind"], ("mid", "inside_low", "inside_high"))]
    return np.concatenate([inside(c), inside(d)])


# ---- (e) vectors steered so that their computed length is a hard divisor -----------------------------------------------------------

STEER_PAIRS = 4000


def steer(x, L):
    """Host arithmetic: for each pair a y with sqrt(x*x + y*y) == L, NaN where the search finds none.  First an s within three
    doubles of L*L whose root is L, then a y within four doubles of sqrt(s - x*x)."""
    x, L = np.asarray(x, dtype=np.float64), np.asarray(L, dtype=np.float64)
    found = np.full(x.shape, np.nan)
    with np.errstate(all="ignore"):
        sq = L * L
        cand = [sq]
        for _ in range(3):
            cand = [np.nextafter(cand[0], -np.inf)] + cand + [np.nextafter(cand[-1], np.inf)]
        for s in cand:
            good = np.sqrt(s) == L
            y0 = np.sqrt(s - x * x)
            ys = [y0]
            for _ in range(4):
                ys = [np.nextafter(ys[0], -np.inf)] + ys + [np.nextafter(ys[-1], np.inf)]
            for y in ys:
                hit = good & np.isnan(found) & (np.sqrt(x * x + y * y) == L)
                found = np.where(hit, y, found)
    return found


@functools.lru_cache(maxsize=None)
def steered_base():
    """dict x, y, L (before rotation, signs and scaling) of the pairs for which a vector was found, and `tried`"""
    rng = random.Random(0xE)
    pairs = [division_pair(rng, 53) for _ in range(STEER_PAIRS)]
    x = np.array([_f(A, -53) for A, _ in pairs])
    L = np.array([_f(B, -53) for _, B in pairs])
    y = steer(x, L)
    keep = ~np.isnan(y)
    return {"x": x[keep], "y": y[keep], "L": L[keep], "tried": STEER_PAIRS}


def _smallest_component_exponent(x, y):
    """j with min(|x|, |y|) * 2^j in [2^-300, 2^-299)"""
    _, e = np.frexp(np.minimum(np.abs(x), np.abs(y)))  # the minimum is in [2^(e-1), 2^e)
    return -300 - (e - 1)


@functools.lru_cache(maxsize=None)
def steered_vectors():
    """dict v [n, 3], L [n] (the length each vector must have), scale (name), hard (the index of the component holding x): the hard
    quotient in each of the three divisions, signs varied; whole vectors times 2^j -- exact, so as hard -- with the length in the
    middle of unit()'s window, on both sides of 0.0001 (2^-13), just under 2^300, and with the smallest component just above 2^-300 (then the vector is left alone)."""
    base = steered_base()
    rng = np.random.default_rng(0xE)
    x, y, L = base["x"], base["y"], base["L"]
    zero = np.zeros_like(x)
    vs, Ls, scales, hard = [], [], [], []
    for name, j in (("mid", np.zeros(len(x), dtype=np.int64)), ("about_1e-4", np.full(len(x), -13)), ("under_2^300", np.full(len(x), 300)),
                    ("component_at_2^-300", _smallest_component_exponent(x, y))):
        for k, comps in enumerate(((x, y, zero), (y, zero, x), (zero, x, y))):
            v = np.ldexp(np.stack(comps, axis=1), j[:, None]) * rng.choice([-1.0, 1.0], (len(x), 3))
            vs.append(v), Ls.append(np.ldexp(L, j)), scales.extend([name] * len(x)), hard.extend([(0, 2, 1)[k]] * len(x))
    return {"v": np.concatenate(vs), "L": np.concatenate(Ls), "scale": np.array(scales), "hard": np.array(hard)}


# ---- (f) window and threshold edges, as explicit values ---------------------------------------------------------------------------

def below(v):
    return float(np.nextafter(v, -np.inf))


def above(v):
    return float(np.nextafter(v, np.inf))


@functools.lru_cache(maxsize=None)
def vectors_of_length(target):
    """vectors whose computed length is exactly `target`, searched in host arithmetic (the exact reference confirms them in the tests):
    (t, 0, 0) when sqrt(t*t) == t, and two-component ones with x = t k / 8"""
    out = []
    with np.errstate(all="ignore"):
        if np.sqrt(np.float64(target) * np.float64(target)) == target:
            out.append((target, 0.0, 0.0))
        xs = np.array([target * k / 8 for k in range(1, 8)])
        ys = steer(xs, np.full(len(xs), target))
    out += [(float(x), float(y), 0.0) for x, y in zip(xs, ys) if not math.isnan(y)]
    assert out, target
    return tuple(out)


@functools.lru_cache(maxsize=None)
def unit_edges():
    """dict v [n, 3], what (one name per vector)"""
    v, what = [], []
    tiny_in, tiny_out = 2.0 ** -300, 2.0 ** -301
    for tiny, name in ((tiny_in, "2^-300"), (tiny_out, "2^-301"), (below(tiny_in), "below_2^-300"), (5e-324, "denormal"), (2.0 ** -1022, "min_normal")):
        for pos in range(3):
            for sign in (1.0, -1.0):
                rec = [0.6, -0.8, 0.75]
                rec[pos] = sign * tiny
                v.append(rec), what.append("component_" + name)
    for x, name in ((below(2.0 ** 300), "below_2^300"), (2.0 ** 300, "2^300"), (above(2.0 ** 300), "above_2^300")):
        for pos in range(3):
            rec = [0.0, 0.0, 0.0]
            rec[pos] = -x if pos == 1 else x
            v.append(rec), what.append("length_" + name)
    for target, name in ((0.0001, "1e-4"), (above(0.0001), "above_1e-4"), (below(0.0001), "below_1e-4")):
        for x, y, z in vectors_of_length(target):
            v += [[x, y, z], [-y, z, x], [-0.0, -x, y]]
            what += ["length_" + name] * 3
    for pos in range(3):
        for zero in (0.0, -0.0):
            for scale in (1.0, 2.0 ** -20):   # divided, and left alone
                rec = [0.28 * scale, -0.96 * scale, 0.5 * scale]
                rec[pos] = zero
                v.append(rec), what.append("signed_zero")
    for zeros in ((0.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (0.0, 0.0, 3.0), (-0.0, 2.0 ** -40, -0.0)):
        v.append(list(zeros)), what.append("signed_zero")
    return {"v": np.array(v), "what": np.array(what)}


FOURTH_FIELD_EDGES = (2.0 ** -300, below(2.0 ** -300), below(2.0 ** 300), 2.0 ** 300)

# records from outside the windows, to put into one lane of a wave that is otherwise inside: (x, y, z, w)
OUTSIDE_RECORDS = (
    ("denormal_component", (0.6, 5e-324, -0.8, 2.25)),
    ("2^300", (2.0 ** 300, 0.0, 0.0, 2.25)),
    ("nan", (float("nan"), 0.5, 0.5, 2.25)),
    ("fourth_zero", (0.6, 0.0, -0.8, 0.0)),
    ("fourth_2^-301", (0.28, -0.96, 0.0, 2.0 ** -301)),
)
REPLACED_LANES = (0, 31, 32, 63)
