"""Device division, square root and unit() on worst-case roundings, judged by exact integer arithmetic.

Random operands leave the exact result some 2^-22 ulp from the nearest rounding boundary at best; a sequence that is one ulp off only
within 2^-30 ulp of a midpoint passes them.  The families of tests/hard_roundings.py sit 2^-49 ulp (division) and 2^-30 ulp (square
root) from a midpoint, on both sides, at every result precision from one bit (the smallest denormals) to 53, and at the exact edges
of the windows in which sqrt_exact and unit() (csrc/trt_device.hpp) take their short paths.  The judge, tests/exact_ieee.py, is Python
integers: it shares no floating-point unit with the device, the host or the oracle, and the CPU tests below pin it to the latter two.

Both self-test kernels run 256-thread blocks, so records 64k .. 64k+63 are one wave: the layouts of the unit() tests rely on that."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_ieee as X
import hard_roundings as H
import support as T

WAVE = H.WAVE
DIVISION_FAMILIES = {"hard": H.division_hard, "threshold": H.division_threshold, "exact": H.division_exact}
SQRT_FAMILIES = {"closed_form": H.sqrt_closed_form, "modular": H.sqrt_modular, "exact_and_denormal": H.sqrt_exact_and_denormal}


# ---- the exact references, formed once per process and left unchanged ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def exact_quotients(name):
    f = DIVISION_FAMILIES[name]()
    return X.div_array(f["a"], f["b"])


@functools.lru_cache(maxsize=None)
def exact_roots(name):
    f = DIVISION_FAMILIES[name]() if name in DIVISION_FAMILIES else SQRT_FAMILIES[name]()
    return X.sqrt_array(f["a"] if name in DIVISION_FAMILIES else f["x"])


@functools.lru_cache(maxsize=None)
def exact_steered():
    """(normalised [n, 3], length [n]) of every steered vector"""
    return X.unit_array(H.steered_vectors()["v"])


@functools.lru_cache(maxsize=None)
def exact_inside_roots():
    return X.sqrt_array(H.sqrt_inside_window())


def exact_records(records):
    """[n, 4] (x, y, z, w) -> [n, 4] (unit(x, y, z), sqrt(w))"""
    u, _ = X.unit_array(records[:, :3])
    return np.concatenate([u, X.sqrt_array(records[:, 3])[:, None]], axis=1)


@functools.lru_cache(maxsize=None)
def uniform_records():
    """(records [n, 4], exact [n, 4]): every steered vector -- all inside unit()'s window -- with the hard square-root arguments
    inside sqrt_exact's window as fourth fields, so that every wave takes both short paths"""
    v, w = H.steered_vectors()["v"], H.sqrt_inside_window()
    n = len(v)
    assert n >= len(w) and n <= 1 << 18
    idx = np.arange(n) % len(w)
    return np.concatenate([v, w[idx, None]], axis=1), np.concatenate([exact_steered()[0], exact_inside_roots()[idx, None]], axis=1)


def host_unit(v):
    """the numpy expression of test_lean_normalisation_and_sqrt_equal_the_plain_operators (tests/test_gpu_parity.py)"""
    with np.errstate(all="ignore"):
        length = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        return np.where((length > 0.0001)[:, None], v[:, :3] / length[:, None], v[:, :3])


def first_difference(same, *columns):
    """for an assertion message: how many differ, and the first record that does, in hex"""
    bad = np.argwhere(~np.asarray(same).reshape(len(same), -1).all(axis=1)).ravel()
    if not len(bad):
        return "none"
    i = int(bad[0])
    return f"{len(bad)} differ; first at {i}: " + " | ".join(" ".join(float(x).hex() for x in np.atleast_1d(c[i])) for c in columns)


# ---- CPU: the reference is right, the cases are what they claim, and they bite --------------------------------------------------------

def test_rn_rounds_fractions_to_nearest_even():
    """rn() on values whose rounding is known without arithmetic: ties go to even at 53 bits and at a denormal's precision, the
    overflow threshold 2^1024 - 2^970 is the first value that gives infinity, half the smallest denormal goes to zero with the
    caller's sign"""
    two = Fraction(2)
    assert X.rn(Fraction(1, 3)) == float.fromhex("0x1.5555555555555p-2") and X.rn(Fraction(-2, 3)) == float.fromhex("-0x1.5555555555555p-1")
    assert X.rn(1 + two ** -53) == 1.0 and X.rn(1 + 3 * two ** -53) == float.fromhex("0x1.0000000000002p+0")
    assert X.rn(1 + two ** -53 + two ** -200) == float.fromhex("0x1.0000000000001p+0")
    assert X.rn(two ** 1024 - two ** 970) == math.inf and X.rn(two ** 1024 - two ** 970 - 1) == float.fromhex("0x1.fffffffffffffp+1023")
    assert X.rn(-(two ** 2000)) == -math.inf
    assert X.rn(two ** -1075) == 0.0 and X.rn(two ** -1075 + two ** -1200) == 5e-324 and X.rn(3 * two ** -1075) == 1e-323
    assert X.rn(two ** -1022 - two ** -1075) == float.fromhex("0x1p-1022")  # the largest denormal's upper midpoint: a tie to the even normal
    assert X.rn(5 * two ** -1076) == 5e-324 and X.rn(7 * two ** -1076) == 1e-323
    assert math.copysign(1.0, X.rn(Fraction(0), 1)) == -1.0 and math.copysign(1.0, X.rn(Fraction(0))) == 1.0
    assert X.sqrt(2.0) == float.fromhex("0x1.6a09e667f3bcdp+0") and X.sqrt(5e-324) == float.fromhex("0x1p-537") and X.sqrt(9.0) == 3.0
    assert math.isnan(X.sqrt(-1.0)) and X.to_bits(X.sqrt(-0.0)) == X.SIGN and math.isnan(X.div(0.0, -0.0)) and X.div(-1.0, 0.0) == -math.inf
    assert X.add(1.0, -1.0) == 0.0 and X.to_bits(X.add(1.0, -1.0)) == 0 and X.to_bits(X.add(-0.0, -0.0)) == X.SIGN
    assert X.unit(3.0, 0.0, -4.0) == (0.6, 0.0, -0.8) and X.unit(3e-5, -0.0, 4e-5) == (3e-5, -0.0, 4e-5)


def test_the_exact_reference_equals_the_host_arithmetic_and_the_oracle():
    """Bit for bit on every generated case and on 2^16 random ones: division and square root against numpy's and against the oracle's
    (trt_oracle_div_sqrt), products and sums against numpy's, unit() against the numpy expression of the random test.  This pins
    the reference on a machine where it can be checked; on the device it then stands alone."""
    rng = np.random.default_rng(11)
    n = 1 << 16
    ra = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.uniform(-30, 30, n)
    rb = rng.uniform(0.5, 1.0, n) * 10.0 ** rng.uniform(-30, 30, n) * rng.choice([-1.0, 1.0], n)
    ra[:4096] *= 1e-300                                     # products and quotients that go denormal, sums of denormals
    rb[2048:8192] *= 1e270
    pairs = [(f()["a"], f()["b"], exact_quotients(name)) for name, f in DIVISION_FAMILIES.items()] + [(ra, rb, X.div_array(ra, rb))]
    lib = T.oracle()
    with np.errstate(all="ignore"):
        for a, b, exact in pairs:
            assert X.same_bits(exact, a / b).all(), first_difference(X.same_bits(exact, a / b), a, b, exact, a / b)
            oq, oroot = np.empty_like(a), np.empty_like(a)
            lib.trt_oracle_div_sqrt(a.ctypes.data, b.ctypes.data, len(a), oq.ctypes.data, oroot.ctypes.data)
            assert X.same_bits(exact, oq).all(), first_difference(X.same_bits(exact, oq), a, b, exact, oq)
        roots = [(f()["a"], exact_roots(name)) for name, f in DIVISION_FAMILIES.items()] + [(f()["x"], exact_roots(name)) for name, f in SQRT_FAMILIES.items()]
        for x, exact in roots + [(np.abs(ra), X.sqrt_array(np.abs(ra)))]:
            assert X.same_bits(exact, np.sqrt(x)).all(), first_difference(X.same_bits(exact, np.sqrt(x)), x, exact, np.sqrt(x))
            oq, oroot = np.empty_like(x), np.empty_like(x)
            lib.trt_oracle_div_sqrt(x.ctypes.data, x.ctypes.data, len(x), oq.ctypes.data, oroot.ctypes.data)
            assert X.same_bits(exact, oroot).all(), first_difference(X.same_bits(exact, oroot), x, exact, oroot)
        prod = X.doubles([X.mul_bits(p, q) for p, q in zip(X.patterns(ra), X.patterns(rb))])
        total = X.doubles([X.add_bits(p, q) for p, q in zip(X.patterns(ra), X.patterns(rb * 1e-3))])
        assert X.same_bits(prod, ra * rb).all() and X.same_bits(total, ra + rb * 1e-3).all()
        special = H.division_exact()
        sa, sb = special["a"], special["b"]
        assert X.same_bits(X.doubles([X.mul_bits(p, q) for p, q in zip(X.patterns(sa), X.patterns(sb))]), sa * sb).all()
        assert X.same_bits(X.doubles([X.add_bits(p, q) for p, q in zip(X.patterns(sa), X.patterns(sb))]), sa + sb).all()
    random_vectors = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-6, 3, (n, 1))
    random_vectors[::5, 1] = 0.0
    random_vectors[:2048] *= 1e-157                          # squares that go denormal
    for v, exact in ((H.steered_vectors()["v"], exact_steered()[0]), (H.unit_edges()["v"], X.unit_array(H.unit_edges()["v"])[0]),
                     (random_vectors, X.unit_array(random_vectors)[0])):
        assert X.same_bits(exact, host_unit(v)).all(), first_difference(X.same_bits(exact, host_unit(v)), v, exact, host_unit(v))


def midpoint_offset_of_quotient(a, b):
    """(p, d): the exact |a / b| has p significant bits once correctly rounded (53, fewer for a denormal; the exponent unbounded
    above), and lies d ulp of that precision above (d > 0) or below the midpoint in its ulp interval"""
    (ma, ea), (mb, eb) = X.decode(X.to_bits(a)), X.decode(X.to_bits(b))
    q = Fraction(ma, mb) * Fraction(2) ** (ea - eb)
    top = q.numerator.bit_length() - q.denominator.bit_length()
    top -= q < Fraction(2) ** top                           # 2^top <= q < 2^(top+1)
    last = max(top, -1022) - 52
    scaled = q / Fraction(2) ** last
    return top - last + 1, scaled - math.floor(scaled) - Fraction(1, 2)


def midpoint_offset_of_root(x, bound_bits):
    """+1 / -1: sqrt(x) lies above / below the midpoint in its 53-bit ulp interval, asserted to be within 2^-bound_bits ulp of it"""
    m, e = X.decode(X.to_bits(x))
    shift = 200 + (e & 1)
    scaled = m << shift
    root = math.isqrt(scaled)                               # root <= sqrt(scaled) < root + 1, some 126 bits
    ulp = 1 << (root.bit_length() - 53)
    mid = root // ulp * ulp + ulp // 2
    assert (abs(root - mid) + 1) << bound_bits <= ulp, float(x).hex()
    assert mid * mid != scaled
    return 1 if scaled > mid * mid else -1


def test_the_cases_are_what_they_claim():
    """By integer arithmetic on the operands themselves:
      (a) every division case lies within 2^-49 ulp of a midpoint of the precision it names, 53 bits or a denormal's fewer;
          every precision from 1 to 53 occurs; at least 0.4 of the cases lie above their midpoint and at least 0.4 below;
      (c) every closed-form square root lies within 2^-30 ulp of a midpoint -- and BELOW it, every one: sqrt is concave, so
          sqrt(1 + m 2^-52) < 1 + m 2^-53 and sqrt(4 - m 2^-51) < 2 - m 2^-53 whatever m is.  The two-sided share is therefore asked
          of the modular family, which exists to supply the cases above;
      (d) every modular square root lies within 2^-30 ulp of a midpoint, at least 0.4 above and at least 0.4 below;
      (e) the steering finds a vector for at least 90 % of the pairs, and every vector kept has exactly the length it was steered to;
      (f) the edge vectors named after a length have that length."""
    d = H.division_hard()
    offsets = [midpoint_offset_of_quotient(a, b) for a, b in zip(d["a"].tolist(), d["b"].tolist())]
    assert [p for p, _ in offsets] == d["p"].tolist() and set(d["p"].tolist()) == set(range(1, 54))
    assert all(abs(off) <= Fraction(1, 1 << H.MIDPOINT_CLAIM_DIV) and off != 0 for _, off in offsets)
    up = sum(off > 0 for _, off in offsets) / len(offsets)
    print(f"(a) {len(offsets)} cases, above the midpoint {up:.3f}, below {1 - up:.3f}")
    assert up >= 0.4 and 1 - up >= 0.4

    c = [midpoint_offset_of_root(x, H.MIDPOINT_CLAIM_SQRT) for x in H.sqrt_closed_form()["x"].tolist()]
    print(f"(c) {len(c)} cases, above the midpoint {c.count(1) / len(c):.3f}, below {c.count(-1) / len(c):.3f}")
    assert c.count(-1) == len(c)
    m = [midpoint_offset_of_root(x, H.MIDPOINT_CLAIM_SQRT) for x in H.sqrt_modular()["x"].tolist()]
    print(f"(d) {len(m)} cases, above the midpoint {m.count(1) / len(m):.3f}, below {m.count(-1) / len(m):.3f}")
    assert m.count(1) / len(m) >= 0.4 and m.count(-1) / len(m) >= 0.4
    for f in (H.sqrt_closed_form(), H.sqrt_modular()):     # the placements are where their names say
        inside = (f["x"] >= 2.0 ** -300) & (f["x"] < 2.0 ** 300)
        assert (inside == np.isin(f["kind"], ("mid", "inside_low", "inside_high"))).all()
        assert ((f["x"][f["kind"] == "inside_low"] < 2.0 ** -298) & (f["x"][f["kind"] == "outside_low"] >= 2.0 ** -302)).all()
        assert ((f["x"][f["kind"] == "inside_high"] >= 2.0 ** 298) & (f["x"][f["kind"] == "outside_high"] < 2.0 ** 302)).all()

    base, sv = H.steered_base(), H.steered_vectors()
    print(f"(e) {len(base['x'])} of {base['tried']} pairs steered ({len(base['x']) / base['tried']:.3f}), {len(sv['v'])} vectors")
    assert len(base["x"]) >= 0.9 * base["tried"]
    _, length = exact_steered()
    assert np.array_equal(length.view(np.uint64), sv["L"].view(np.uint64))
    hard = np.abs(sv["v"][np.arange(len(sv["v"])), sv["hard"]])   # the component that holds x: x / L is an (a) case of 53 bits
    mid = sv["scale"] == "mid"
    assert all(p == 53 and abs(off) <= Fraction(1, 1 << H.MIDPOINT_CLAIM_DIV) for p, off in
               (midpoint_offset_of_quotient(a, b) for a, b in zip(hard[mid].tolist(), sv["L"][mid].tolist())))
    # the scalings put the vectors where they say, all inside unit()'s window
    nonzero = np.where(sv["v"] == 0.0, np.inf, np.abs(sv["v"])).min(axis=1)
    assert (sv["L"] < 2.0 ** 300).all() and (nonzero >= 2.0 ** -300).all()
    assert (sv["L"][sv["scale"] == "under_2^300"] >= 2.0 ** 299).all() and (nonzero[sv["scale"] == "component_at_2^-300"] < 2.0 ** -299).all()
    about = sv["L"][sv["scale"] == "about_1e-4"]
    assert 0.2 < (about > 0.0001).mean() < 0.8

    e = H.unit_edges()
    _, length = X.unit_array(e["v"])
    for name, want in (("length_1e-4", 0.0001), ("length_above_1e-4", H.above(0.0001)), ("length_below_1e-4", H.below(0.0001)),
                       ("length_below_2^300", H.below(2.0 ** 300)), ("length_2^300", 2.0 ** 300)):
        got = length[e["what"] == name]
        assert len(got) >= 3 and (got == want).all(), name


def test_the_cases_bite():
    """A quotient or root formed with a 64-bit significand and rounded again to binary64 -- "nearly" correctly rounded -- differs
    from the reference on at least a third of (a), (c) and (d), and on under 1 % of random operands."""
    if np.finfo(np.longdouble).nmant != 63:
        pytest.skip("np.longdouble has no 64-bit significand here: no double rounding to show")
    ld = np.longdouble
    rng = np.random.default_rng(12)
    n = 1 << 16
    ra, rb = rng.uniform(0.0, 1.0, n) * 10.0 ** rng.uniform(-30, 30, n), rng.uniform(0.5, 1.0, n) * 10.0 ** rng.uniform(-30, 30, n)
    with np.errstate(all="ignore"):
        d = H.division_hard()
        twice = (d["a"].astype(ld) / d["b"].astype(ld)).astype(np.float64)
        share = {"(a)": (~X.same_bits(twice, exact_quotients("hard"))).mean()}
        for tag, name in (("(c)", "closed_form"), ("(d)", "modular")):
            x = SQRT_FAMILIES[name]()["x"]
            share[tag] = (~X.same_bits(np.sqrt(x.astype(ld)).astype(np.float64), exact_roots(name))).mean()
        random_div = (~X.same_bits((ra.astype(ld) / rb.astype(ld)).astype(np.float64), X.div_array(ra, rb))).mean()
        random_root = (~X.same_bits(np.sqrt(ra.astype(ld)).astype(np.float64), X.sqrt_array(ra))).mean()
    print("double rounding differs on", {k: round(float(v), 4) for k, v in share.items()}, "random division", random_div, "random root", random_root)
    assert all(v >= 1 / 3 for v in share.values()), share
    assert random_div < 0.01 and random_root < 0.01


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from terminalraytracer_amd import hip
    c = hip.Context(0)
    yield c
    c.close()


def run_unit(ctx, records):
    assert len(records) <= 1 << 18
    with np.errstate(all="ignore"):
        return ctx.selftest_unit(records)


def assert_records(fast, ref, exact, records, what):
    for got, name in ((fast, "lean"), (ref, "plain")):
        same = X.same_bits(got, exact)
        assert same.all(), f"{what}, {name} code against the exact reference: " + first_difference(same, records, got, exact)


@pytest.fixture(scope="module")
def uniform_run(ctx):
    records, _ = uniform_records()
    return run_unit(ctx, records)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(DIVISION_FAMILIES))
def test_device_division_of_hard_cases_is_correctly_rounded(ctx, family):
    """the compiler's `/` on (a) and (b): quotients next to a midpoint at 53 bits, in the last binade, past it, denormal at every
    precision, with denormal operands; exact ones and their neighbours; every special.  (The roots of the numerators are judged too.)"""
    f = DIVISION_FAMILIES[family]()
    a, b = f["a"], f["b"]
    assert len(a) <= 1 << 18
    q, r = ctx.selftest_div_sqrt(a, b)
    same = X.same_bits(q, exact_quotients(family))
    assert same.all(), first_difference(same, a, b, q, exact_quotients(family))
    same = X.same_bits(r, exact_roots(family))
    assert same.all(), first_difference(same, a, r, exact_roots(family))


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(SQRT_FAMILIES))
def test_device_sqrt_of_hard_cases_is_correctly_rounded(ctx, family):
    """the compiler's sqrt on (c) and (d): roots next to a midpoint from both sides, in the middle of the range, about 2^+-300 and at
    the ends of the range; perfect squares and their neighbours; denormals; specials.  x / 1.0 must be x."""
    x = SQRT_FAMILIES[family]()["x"]
    assert len(x) <= 1 << 18
    q, r = ctx.selftest_div_sqrt(x, np.ones_like(x))
    same = X.same_bits(r, exact_roots(family))
    assert same.all(), first_difference(same, x, r, exact_roots(family))
    same = X.same_bits(q, x)
    assert same.all(), first_difference(same, x, q)


@pytest.mark.gpu
def test_short_paths_on_uniform_waves_of_hard_cases(ctx, uniform_run):
    """Every wave inside both windows: the shared-reciprocal divisions of unit() meet the hard quotient in each of their three
    places, at a length in the middle of the window, on both sides of 0.0001, just under 2^300, and with a component just above
    2^-300; sqrt_exact meets the hard roots of (c) and (d).  Lean code, plain operators and exact reference: one and the same."""
    records, exact = uniform_records()
    fast, ref = uniform_run
    assert_records(fast, ref, exact, records, "uniform waves")
    alone = ~(exact_steered()[1] > 0.0001)                  # left alone: the operand's own bits, -0.0 included
    assert alone.any() and (fast[alone, :3].view(np.uint64) == records[alone, :3].view(np.uint64)).all()


@pytest.mark.gpu
def test_one_lane_outside_the_window_changes_no_other_lane(ctx, uniform_run):
    """The same records with ONE lane of every wave replaced by a record from outside a window -- a denormal component, a length of
    2^300, a NaN (unit() then takes the plain operators for the whole wave), a fourth field of 0.0 or 2^-301 (sqrt_exact selects
    per lane) -- in lane 0, 31, 32 or 63.  Every other record must give the bits it gave in the uniform layout, and the replaced
    ones those of the exact reference."""
    records, exact = uniform_records()
    records, exact = records.copy(), exact.copy()
    replacements = np.array([r for _, r in H.OUTSIDE_RECORDS])
    exact_replacements = exact_records(replacements)
    waves = np.arange(len(records) // WAVE)
    at = waves * WAVE + np.array(H.REPLACED_LANES)[waves % len(H.REPLACED_LANES)]
    which = (waves // len(H.REPLACED_LANES)) % len(replacements)
    records[at], exact[at] = replacements[which], exact_replacements[which]
    fast, ref = run_unit(ctx, records)
    assert_records(fast, ref, exact, records, "one lane outside")
    kept = np.ones(len(records), dtype=bool)
    kept[at] = False
    same = X.same_bits(fast[kept], uniform_run[0][kept])
    assert same.all(), first_difference(same, records[kept], fast[kept], uniform_run[0][kept])


@pytest.mark.gpu
def test_lengths_on_both_sides_of_the_threshold_share_a_wave(ctx):
    """Waves inside the window whose lanes alternate between vectors that are divided (length in [0.5, 1)) and vectors that are
    left alone or not according to their length about 0.0001: the lanes "divided" by 1.0 must return the operand's own bits, -0.0
    included, next to lanes that divide by a hard length.  Then the same with the vectors whose length is exactly 0.0001, its
    successor or its predecessor, and those with signed zeros, in lanes of their own."""
    sv = H.steered_vectors()
    n = min(int((sv["scale"] == "mid").sum()), 8192)
    divided, about = np.flatnonzero(sv["scale"] == "mid")[:n], np.flatnonzero(sv["scale"] == "about_1e-4")[-n:]
    order = np.stack([divided, about], axis=1).ravel()
    edges = H.unit_edges()
    pick = np.flatnonzero(np.char.startswith(edges["what"], "length_") & np.char.endswith(edges["what"], "1e-4") | (edges["what"] == "signed_zero"))
    records = np.concatenate([sv["v"][order], np.full((len(order), 1), 2.25)], axis=1)
    exact = np.concatenate([exact_steered()[0][order], np.full((len(order), 1), 1.5)], axis=1)
    lanes = (np.arange(len(pick)) * (WAVE + 5)) % (len(records) - WAVE) + WAVE   # one per wave, the lane moving on by five
    records[lanes, :3] = edges["v"][pick]
    exact[lanes, :3] = X.unit_array(edges["v"][pick])[0]
    length = X.unit_array(records[:, :3])[1]
    per_wave = (length[: len(length) // WAVE * WAVE] > 0.0001).reshape(-1, WAVE).mean(axis=1)
    assert (per_wave > 0).all() and (per_wave < 1).all()    # every wave holds both kinds
    fast, ref = run_unit(ctx, records)
    assert_records(fast, ref, exact, records, "both sides of 0.0001")
    alone = ~(length > 0.0001)
    assert (fast[alone, :3].view(np.uint64) == records[alone, :3].view(np.uint64)).all()
    assert (np.signbit(records[alone, :3]) & (records[alone, :3] == 0.0)).any()


@pytest.mark.gpu
def test_exact_window_boundaries_in_a_single_lane(ctx):
    """One lane of a wave that is otherwise inside holds an exact boundary value: a component of 2^-300 (inside) or 2^-301 (outside),
    a length equal to the double below 2^300 (inside) or to 2^300 (outside), and for sqrt_exact's argument 2^-300, its predecessor,
    the predecessor of 2^300 and 2^300; each in lane 0, 31, 32 and 63.  Then all of them side by side."""
    base, base_exact = uniform_records()
    edges = H.unit_edges()
    singles = [np.append(v, 2.25) for v in edges["v"]] + [np.array([0.6, 0.0, -0.8, w]) for w in H.FOURTH_FIELD_EDGES]
    singles = np.array(singles)
    exact_singles = exact_records(singles)
    count = len(singles) * len(H.REPLACED_LANES)
    records, exact = base[: count * WAVE].copy(), base_exact[: count * WAVE].copy()
    at = np.arange(count) * WAVE + np.tile(H.REPLACED_LANES, len(singles))
    records[at], exact[at] = np.repeat(singles, len(H.REPLACED_LANES), axis=0), np.repeat(exact_singles, len(H.REPLACED_LANES), axis=0)
    records, exact = np.concatenate([records, singles]), np.concatenate([exact, exact_singles])
    fast, ref = run_unit(ctx, records)
    assert_records(fast, ref, exact, records, "exact boundaries")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 257, 64 * 37 + 1])
def test_partial_waves_take_the_same_results(ctx, uniform_run, n):
    """n records of (e): the lanes past the end are inactive and must neither push the wave off the short path nor change a result"""
    records, exact = uniform_records()
    fast, ref = run_unit(ctx, records[:n])
    assert_records(fast, ref, exact[:n], records[:n], f"{n} records")
    assert X.same_bits(fast, uniform_run[0][:n]).all()
