"""unit_round() of csrc/trt_device.hpp, the normalisation of the render rounds: ONE window on the squared length, 2^-26 <= s < 2^300,
sends the WAVE the short way (no range guard, nothing selected); any lane outside it, or with a component that is neither zero nor
at least 2^-300 in magnitude, sends its wave through unit() with every guard.  Either way the bits are those of the plain operators
(unit_reference), lane by lane: a single odd lane must change the way of its wave and nothing in the other 63.  Then frames: the
SYNTH scenes in the plain, the decoupled and the patch kernels, one of them under cameras whose primary directions are outside the
window, against the oracle's frames and ray counts.  A wave that took the short way also skips the unit test of the ray families'
membership (path_cell, shadow_stage in csrc/trt_rounds.hpp), which it is known to pass: the traces that fall back to the sweep are,
to the count, those of the parent commit, whose kernels ran the test for every ray."""
import numpy as np
import pytest

import support as T
from support import COMPACT, PLAIN, bits
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

pytestmark = pytest.mark.gpu

PATCHES = "patches"
VARIANTS = [PLAIN, COMPACT, PATCHES]
LOW, HIGH = 2.0 ** -26, 2.0 ** 300  # the window on the squared length


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.enable_counters(False)
        c.set_path_patches(-1)
        c.set_path_grids_min_spheres(12)
        c.set_compaction(-1)


def square(v):
    """the squared length as the device forms it: (xx + yy) + zz, one rounding per operation"""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def with_square(target):
    """a vector (x, y, 0) whose squared length is `target` to the bit: x a few doubles below the root, y the root of what is missing
    (its own rounding error is far below half an ulp of the target)"""
    x = np.sqrt(np.float64(target))
    for _ in range(3):
        x = np.nextafter(x, 0.0)
    y = np.sqrt(np.float64(target) - x * x)
    v = np.array([x, y, 0.0])
    assert square(v) == target and y > 0.0, (target, v)
    return v


def odd_lanes():
    """[(name, vector, plain)]: the lanes of the issue's list; `plain`: inside the window with whole components (the wave may stay short)"""
    down, up = (lambda x: np.nextafter(np.float64(x), 0.0)), (lambda x: np.nextafter(np.float64(x), np.inf))
    tiny = 2.0 ** -301
    out = [("s one ulp below 2^-26", with_square(down(LOW)), False), ("s = 2^-26", with_square(LOW), True),
           ("s = 2^-26, one component", np.array([0.0, 2.0 ** -13, 0.0]), True), ("s one ulp above 2^-26", with_square(up(LOW)), True),
           ("s one ulp below 2^300", with_square(down(HIGH)), True), ("s = 2^300", with_square(HIGH), False),
           ("s = 2^300, one component", np.array([0.0, 0.0, -2.0 ** 150]), False)]
    for k, x in enumerate((down(down(1e-4)), down(1e-4), np.float64(1e-4), up(1e-4), up(up(1e-4)))):
        out.append((f"len about 1e-4 ({k - 2:+d} ulp)", np.array([0.0, -x, 0.0]), False))
    out.append(("len about 1e-4, three components", np.array([6e-5, -6e-5, 5.2915e-5]), False))
    out += [("zero vector", np.zeros(3), False), ("minus zero vector", np.array([-0.0, -0.0, -0.0]), False),
            ("one zero component", np.array([0.6, 0.0, -0.8]), True), ("two zero components", np.array([0.0, 1.0, 0.0]), True),
            ("two zero components, not unit", np.array([0.0, 0.0, -3.7]), True),
            ("a component of 2^-301", np.array([0.9, tiny, -0.7]), False), ("a component of 2^-300", np.array([0.9, 2 * tiny, -0.7]), True),
            ("a denormal component", np.array([-1.1, 0.4, 4.9e-324]), False), ("a larger denormal component", np.array([1e-310, 1.0, 0.2]), False),
            ("NaN component", np.array([0.3, np.nan, 0.5]), False), ("infinite component", np.array([0.3, 0.5, -np.inf]), False),
            ("minus zero beside values", np.array([-0.0, 0.5, -0.25]), True), ("two minus zeros", np.array([-0.0, -0.0, 2.0]), True),
            ("minus zero, too short to divide", np.array([-0.0, 5e-5, 0.0]), False)]
    for name, v, plain in out:
        s = square(v)
        whole = all(c == 0.0 or abs(c) >= 2.0 ** -300 for c in v)
        assert plain == bool(LOW <= s < HIGH and whole), name  # the list says what it means to
    return out


def plain_vectors(rng, n):
    """directions, offsets to lights, normals: lengths between 1e-3 and 1e3, whole components"""
    v = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
    assert ((square(v) >= LOW) & (square(v) < HIGH)).all()
    return v


def run(ctx, vectors):
    rec = np.zeros((len(vectors), 4))
    rec[:, :3] = vectors
    rec[:, 3] = 2.0
    with np.errstate(all="ignore"):
        fast, ref = ctx.selftest_unit(rec)
        s = square(rec)
        length = np.sqrt(s)
        host = np.where((length > 0.0001)[:, None], rec[:, :3] / length[:, None], rec[:, :3])
    return fast[:, :3], ref[:, :3], host


def same(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def test_one_odd_lane_sends_its_wave_the_long_way_and_changes_no_other_lane(ctx):
    """Waves of 63 plain lanes and one odd one, the odd one first, in the middle and last: every wave of the one launch is a batch of
    its own (64 records a wave).  The plain lanes' results must be what the same vectors give in a wave of plain lanes only."""
    rng = np.random.default_rng(27)
    base = plain_vectors(rng, 64)
    cases = odd_lanes()
    waves, where = [base], [(None, None)]
    for name, v, _ in cases:
        for lane in (0, 37, 63):
            w = base.copy()
            w[lane] = v
            waves.append(w), where.append((name, lane))
    fast, ref, host = run(ctx, np.concatenate(waves))
    ok = same(fast, ref).all(axis=1) & same(ref, host).all(axis=1)
    bad = np.argwhere(~ok)[:, 0]
    assert ok.all(), [(where[i // 64], int(i % 64)) for i in bad[:5]]
    fast = fast.reshape(-1, 64, 3)
    for k, (name, lane) in enumerate(where[1:], 1):
        others = np.arange(64) != lane
        assert np.array_equal(bits(fast[k][others]), bits(fast[0][others])), (name, lane)
    # the sign of a zero numerator is the quotient's
    for name, v, _ in cases:
        k = 1 + 3 * [c[0] for c in cases].index(name)
        zero = v == 0.0
        assert np.array_equal(np.signbit(fast[k][0][zero]), np.signbit(v[zero])), name


def test_batches_of_65_leave_a_wave_of_one_lane(ctx):
    """65 records: a full wave and a wave with ONE active lane (the votes must not count the 63 inactive ones).  The odd lane in the
    full wave (the lone lane plain) and as the lone lane (the full wave plain)."""
    rng = np.random.default_rng(65)
    base = plain_vectors(rng, 65)
    alone, _, _ = run(ctx, base)
    for name, v, _ in odd_lanes():
        for lane in (5, 64):
            w = base.copy()
            w[lane] = v
            fast, ref, host = run(ctx, w)
            assert same(fast, ref).all() and same(ref, host).all(), (name, lane)
            others = np.arange(65) != lane
            assert np.array_equal(bits(fast[others]), bits(alone[others])), (name, lane)


def test_random_vectors_with_exponents_all_over_the_range(ctx):
    """2^16 vectors, every component with an exponent of its own drawn from [-310, 310]: most waves hold a lane outside the window; in
    a second launch each WAVE shares one exponent, so that whole waves are plain, whole waves are not, and some straddle an end"""
    rng = np.random.default_rng(310)
    n = 1 << 16
    mant = rng.uniform(1.0, 2.0, (n, 3)) * rng.choice([-1.0, 1.0], (n, 3))
    with np.errstate(all="ignore"):
        per_lane = mant * 2.0 ** rng.integers(-310, 311, (n, 3)).astype(np.float64)
        per_wave = mant * 2.0 ** np.repeat(rng.integers(-310, 311, n // 64), 64).astype(np.float64)[:, None]
    for what, v in (("an exponent a component", per_lane), ("an exponent a wave", per_wave)):
        fast, ref, host = run(ctx, v)
        ok = same(fast, ref).all(axis=1)
        assert ok.all(), (what, int((~ok).sum()), v[np.argwhere(~ok)[0][0]])
        ok = same(ref, host).all(axis=1)
        assert ok.all(), (what, int((~ok).sum()), v[np.argwhere(~ok)[0][0]])
    plain = (square(per_wave) >= LOW) & (square(per_wave) < HIGH)
    whole = plain.reshape(-1, 64).all(axis=1)
    assert 0.2 < whole.mean() < 0.8 and (~plain).reshape(-1, 64).all(axis=1).any()  # both ways were taken by whole waves


# ---- frames ----

W, H, BOUNCES, SPP = 96, 54, 8, 3


def tiny_basis(cam):
    """basis vectors of length 1e-5 (the primary directions are then about minus the eye's position: TRT.c:1005)"""
    out = cam.copy()
    out[0:9] *= 1e-5
    return out


def tiny_basis_and_eye(cam):
    """... and the eye 3e-5 from the origin: every primary direction is shorter than 1e-4 and is left as it is (TRT.c:439-450); the
    waves of the first round take unit()'s way"""
    out = tiny_basis(cam)
    out[9:12] = [1e-5, 2e-5, -2e-5]
    return out


FRAMES = [("8 spheres", 8, None), ("12 spheres", 12, None), ("64 spheres", 64, None),
          ("64 spheres, basis 1e-5", 64, tiny_basis), ("64 spheres, basis 1e-5, eye 3e-5 from the origin", 64, tiny_basis_and_eye)]


# `swept_traces` of the counting instantiations (plain, decoupled, patches) for these frames, from a build of the PARENT commit
# (every normalisation through unit(), the unit test of the membership always run) -- not from the tree under test
PARENT_SWEPT = {"8 spheres": (6, 6, 6), "12 spheres": (5, 5, 5), "64 spheres": (13, 13, 13), "64 spheres, basis 1e-5": (0, 0, 0),
                "64 spheres, basis 1e-5, eye 3e-5 from the origin": (633, 633, 558)}  # (the last one's directions are no unit vectors)


@pytest.fixture(scope="module")
def oracle_frames():
    out = {}
    for name, n, bend in FRAMES:
        cam = T.bench_camera(W, H)
        scene = S.synth_scene(n, T.sky("synth"), bend(cam) if bend else cam)
        with np.errstate(all="ignore"):
            want, st = T.oracle_render(scene, W, H, BOUNCES, SPP)
        out[name] = (scene, want, (st.path_rays, st.shadow_rays))
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", [f[0] for f in FRAMES])
def test_frames_and_ray_counts_are_the_oracles(ctx, oracle_frames, name, variant):
    scene, want, rays = oracle_frames[name]
    if name.endswith("from the origin"):
        first = scene.camera[0:9].reshape(3, 3).T @ np.array([1.0, 1.0, -scene.camera[12]]) - scene.camera[9:12]
        assert square(first) < LOW  # such a camera's directions ARE outside the window
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_compaction(1 if variant == COMPACT else 0 if variant == PLAIN else -1)
    ctx.set_path_patches(1 if variant == PATCHES else 0)
    ctx.set_path_grids_min_spheres(0)
    ctx.set_scene(scene)
    for count in (False, True):  # the shipping instantiation, then the counting one
        ctx.enable_counters(count)
        got = ctx.render_host(scene.camera, hip.RowSet.whole(W, H), BOUNCES, SPP)
        assert variant == PATCHES or ctx.render_variant()["decoupled"] == (variant == COMPACT)
        assert np.array_equal(bits(got), bits(want)), (name, variant, count)
        if count:
            assert ctx.read_counters() == rays
            swept = ctx.read_diagnostics()["swept_traces"]
            print(f"\n{name} {variant}: swept traces {swept}, the parent's {PARENT_SWEPT[name][VARIANTS.index(variant)]}")
            # a wave whose directions come out of unit_round()'s short way skips the unit test of the family membership; that test
            # never decided differently: no trace more and none fewer falls back to the sweep
            assert swept == PARENT_SWEPT[name][VARIANTS.index(variant)]
