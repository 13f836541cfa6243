"""Rays that sit ON the compares of the render rounds (csrc/trt_rounds.hpp: exact_step, trace's ground test, path_cell's membership test,
point_light_search and the closest-hit search behind it), and tiny frames through both render variants.

The rounds' wave votes are taken from the compares' own lane words (csrc/trt_device.hpp, lanes_with); which branch a wave takes hangs on
compares whose operands these rays put on the edge: a discriminant of exactly 0 and one step either side, a hit parameter of +0.0 and
of -0.0, a direction with |d.d - 1| of exactly 2^-40 and one step beyond, a blocker exactly as far as the point light, a ray in the ground
plane and rays whose |d.n| is 1e-5 and one step either side.

Two layers, as in test_candidate_edges.py.  The CPU layer proves the aim: the operands, restated in numpy's binary64 in the kernel's
operation order (no contraction), have the intended values, and the oracle gives the answer the edge implies.  The GPU layer sends the rays
through the production stages (trt_probe_rays_production) -- without a family (the wave sweeps) and as rays of the eye's family from an eye at
their origin (the wave reads its lists) -- and compares with the oracle bit for bit; then one 16 x 8 frame per render variant."""
import functools

import numpy as np
import pytest

import support as T
from support import bits
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S
from test_candidate_edges import same_probe

GRAZED = 0    # sphere 0: centre at the origin, radius 0.5 (r * r = 0.25 exactly)
TOUCHING = 1  # sphere 1: its lowest point IS the point light
LIGHT = np.array([0.0, 3.0, 0.0])
UNIT_TOLERANCE = 9.094947017729282e-13  # 2^-40, the membership tests' |d.d - 1| bound
PLANE_MIN = 0.00001                     # TRT.c:683, :690


@functools.lru_cache(maxsize=None)
def edge_scene():
    sph = T.directed_spheres([[0.0, 0.0, 0.0], [0.0, 3.5, 0.0], [3.0, 0.0, 1.0]], [0.5, 0.5, 0.7])
    d, _ = S.demo_lights()
    pl = np.array([[*LIGHT, 1.0, 0.9, 0.8, 10.0]])
    return S.SceneData(sph, S.demo_ground(), d, pl, T.bench_camera(16, 8), T.sky("synth"))


def steps(x, k):
    """x moved k representable numbers up (k > 0) or down"""
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return float(x)


def discriminant(o, d, c, r):
    """b, disc of exact_step / TRT.c:638-655 in its operation order"""
    o, d, c = (np.asarray(v, dtype=np.float64) for v in (o, d, c))
    oc = o - c
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    a, b = dot(d, d), 2.0 * dot(oc, d)
    cc = dot(oc, oc) - r * r
    return b, b * b - 4.0 * a * cc


@functools.lru_cache(maxsize=None)
def edge_rays():
    """{group: (origin of the group's eye, rays[n, 6])}: every ray of a group starts at the group's origin, or the group has no common origin (None)"""
    groups = {}
    # grazing sphere 0 from (x, 0, -0.5) along +z: b = -1, cc = x^2, disc = 1 - 4 x^2: 0 at x = 0.5, one step of x either side of it
    groups["grazing"] = (None, np.array([[steps(0.5, k), 0.0, -0.5, 0.0, 0.0, 1.0] for k in (-3, -2, -1, 0, 1, 2, 3)]))
    # the hit parameter: +0.0 from a point of the sphere's surface looking inwards (cc = 0, -b = root), -0.0 from one looking along the tangent
    # (b = +0, disc = +0: -b - root = -0.0); the ground's t = +0 from points of the plane, heading into it and out of it
    groups["zero parameter"] = (None, np.array([[0.0, 0.0, -0.5, 0.0, 0.0, 1.0], [0.5, 0.0, 0.0, 0.0, 0.0, 1.0], [0.5, 0.0, 0.0, 0.0, 1.0, 0.0],
                                                [1.0, -2.0, 1.0, 0.0, -1.0, 0.0], [1.0, -2.0, 1.0, 0.0, 1.0, 0.0], [-1.0, -2.0, -1.0, 0.6, -0.8, 0.0]]))
    # directions along z of squared length 1 +- 2^-40 exactly (members of the eye's family) and one step beyond (not), from one eye, at sphere 0
    eye = np.array([0.0, 0.0, -6.0])
    zs = [steps(1.0 + 2.0 ** -41, k) for k in (-1, 0, 1)] + [steps(1.0 - 2.0 ** -41, k) for k in (-1, 0, 1)] + [1.0]
    groups["unit tolerance"] = (eye, np.array([[*eye, 0.0, 0.0, z] for z in zs]))
    # straight down onto the top of sphere 0: the shadow ray of the point light runs up the y axis into sphere 1, which it meets AT the light
    groups["blocker at the light"] = (np.array([0.0, 2.5, 0.0]), np.array([[0.0, 2.5, 0.0, 0.0, -1.0, 0.0], [0.0, 2.5, 0.0, 1e-3, -1.0, 0.0], [0.0, 2.5, 0.0, 0.0, -1.0, -1e-3]]))
    # in the ground plane and parallel to it; then |d.n| = 1e-5 and one step either side, from above and from below, towards the plane
    flat = [[-3.0, -2.0, 0.5, 1.0, 0.0, 0.0], [-3.0, -1.0, 0.5, 1.0, 0.0, 0.0], [-3.0, -2.0, 0.5, 1.0, -0.0, 0.0]]
    for k in (-1, 0, 1):
        flat.append([-3.0, -1.0, 0.5, 1.0, -steps(PLANE_MIN, k), 0.0])
        flat.append([-3.0, -3.0, 0.5, 1.0, steps(PLANE_MIN, k), 0.0])
    groups["ground plane"] = (None, np.array(flat))
    return groups


@functools.lru_cache(maxsize=None)
def oracle_answers():
    scene = edge_scene()
    return {name: T.oracle_probe(scene, rays) for name, (_, rays) in edge_rays().items()}


# ---- the CPU layer: the rays are where they are meant to be ----

def test_grazing_rays_straddle_a_discriminant_of_zero():
    scene, (_, rays), want = edge_scene(), edge_rays()["grazing"], oracle_answers()["grazing"]
    disc = [discriminant(r[:3], r[3:], scene.spheres[GRAZED, :3], scene.spheres[GRAZED, 3])[1] for r in rays]
    assert disc[3] == 0.0 and not np.signbit(disc[3])
    assert all(v > 0.0 for v in disc[:3]) and all(v < 0.0 for v in disc[4:])
    assert disc[2] == 2.0 ** -52 and disc[4] == -(2.0 ** -51)  # one step of the origin: the smallest discriminants either side
    hit = (want["obj"] == 1) & (want["material"][:, :3] == T.index_colour(GRAZED)).all(axis=1)
    assert hit.tolist() == [True] * 4 + [False] * 3  # disc >= 0 meets the sphere (TRT.c:655 rejects disc < 0 only)


def test_zero_hit_parameters_have_both_signs_and_miss():
    scene, (_, rays), want = edge_scene(), edge_rays()["zero parameter"], oracle_answers()["zero parameter"]
    c, r = scene.spheres[GRAZED, :3], scene.spheres[GRAZED, 3]
    b, disc = discriminant(rays[0, :3], rays[0, 3:], c, r)
    t0 = (-b - np.sqrt(disc)) / 2.0
    assert b < 0.0 and t0 == 0.0 and not np.signbit(t0)
    for k in (1, 2):
        b, disc = discriminant(rays[k, :3], rays[k, 3:], c, r)
        t0 = (-b - np.sqrt(disc)) / 2.0
        assert b == 0.0 and disc == 0.0 and t0 == 0.0 and np.signbit(t0), (k, b, disc, t0)
    # t0 > 0 fails for either zero (TRT.c:659): none of the three meets sphere 0 at its own origin; ray 0 goes on through the sphere's inside
    assert not ((want["obj"][:3] == 1) & (want["material"][:3, :3] == T.index_colour(GRAZED)).all(axis=1)).any()
    # origins in the plane: t = 0 / d.n, not above 1e-5 (TRT.c:690), for a numerator of either sign pattern against the denominator
    gp, gn = scene.ground[0:3], scene.ground[3:6]
    for k in (3, 4, 5):
        w = gp - rays[k, :3]
        num, den = (w[0] * gn[0] + w[1] * gn[1]) + w[2] * gn[2], (rays[k, 3] * gn[0] + rays[k, 4] * gn[1]) + rays[k, 5] * gn[2]
        assert num == 0.0 and abs(den) > PLANE_MIN and num / den == 0.0
        assert want["obj"][k] != 2
    assert {bool(np.signbit(rays[k, 4])) for k in (3, 4, 5)} == {True, False}  # the sign test ahead of the division sees both


def test_squared_lengths_sit_on_the_membership_tolerance():
    (eye, rays), want = edge_rays()["unit tolerance"], oracle_answers()["unit tolerance"]
    off = [abs(((r[3] * r[3] + r[4] * r[4]) + r[5] * r[5]) - 1.0) for r in rays]
    assert UNIT_TOLERANCE == 2.0 ** -40
    assert off[1] == 2.0 ** -40 and off[4] == 2.0 ** -40 and off[6] == 0.0
    assert off[2] > 2.0 ** -40 and off[3] > 2.0 ** -40  # one step beyond on either side of one
    assert off[0] <= 2.0 ** -40 and off[5] <= 2.0 ** -40
    assert (want["obj"] == 1).all()


def test_the_blocker_is_exactly_as_far_as_the_light():
    scene, want = edge_scene(), oracle_answers()["blocker at the light"]
    p = want["point"][0]  # the nudged hit point on top of sphere 0
    assert want["obj"][0] == 1 and p[0] == 0.0 and p[2] == 0.0 and 0.5 < p[1] < 0.5 + 2e-6
    # up the y axis sphere 1 (centre 3.5, radius 0.5) is met at y = 3: where the light is
    assert scene.spheres[TOUCHING, 1] - scene.spheres[TOUCHING, 3] == LIGHT[1]
    b, disc = discriminant(p, [0.0, 1.0, 0.0], scene.spheres[TOUCHING, :3], scene.spheres[TOUCHING, 3])
    t0 = (-b - np.sqrt(disc)) / 2.0
    assert abs((p[1] + t0) - LIGHT[1]) <= 2.0 ** -50  # the blocker's hit point and the light agree to the last digits
    assert (want["obj"] == 1).all()


def test_flat_rays_sit_on_the_plane_tests_threshold():
    scene, (_, rays), want = edge_scene(), edge_rays()["ground plane"], oracle_answers()["ground plane"]
    gn = scene.ground[3:6]
    den = np.array([(r[3] * gn[0] + r[4] * gn[1]) + r[5] * gn[2] for r in rays])
    assert (den[:3] == 0.0).all() and np.signbit(rays[2, 4]) and (want["obj"][:3] != 2).all()  # d.n = 0, also from a component of -0.0
    assert [abs(v) > PLANE_MIN for v in den[3:]] == [False, False, False, False, True, True]
    assert abs(den[5]) == PLANE_MIN and abs(den[6]) == PLANE_MIN
    # one step above the threshold the ray meets the plane, from above and from below (the plane has no sides); at and under it, it does not
    assert want["obj"][7] == 2 and want["obj"][8] == 2 and (want["obj"][3:7] != 2).all()


# ---- the GPU layer ----

@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.set_path_grids_min_spheres(0)  # three spheres: the path rays' tables are built all the same
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(edge_rays()))
def test_edge_rays_through_the_production_stages_equal_the_oracle(ctx, group):
    """every ray of a group, bit for bit: in a wave that sweeps (no family); in a wave that is given the eye's family from an eye at the group's origin
    (members read the eye's lists; where the group has no common origin, or a ray's direction is beyond the tolerance, the vote sends the wave to
    the sweep); and each ray alone in its wave, so that every vote is the ray's own"""
    scene = edge_scene()
    eye, rays = edge_rays()[group]
    want = oracle_answers()[group]
    ctx.set_scene(scene)
    same_probe(ctx.probe_rays_production(scene.camera, rays), want, (group, "no family"))
    cam = scene.camera.copy()
    if eye is not None:
        cam[9:12] = eye
    same_probe(ctx.probe_rays_production(cam, rays, np.zeros(len(rays), dtype=np.int32)), want, (group, "the eye's family"))
    for k in range(len(rays)):
        alone = {name: a[k:k + 1] for name, a in want.items()}
        cam[9:12] = rays[k, :3]
        same_probe(ctx.probe_rays_production(cam, rays[k:k + 1], np.zeros(1, dtype=np.int32)), alone, (group, k, "alone, the eye's family"))
        same_probe(ctx.probe_rays_production(cam, rays[k:k + 1]), alone, (group, k, "alone, no family"))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", [T.PLAIN, T.COMPACT], ids=["plain", "decoupled"])
def test_a_tiny_frame_of_each_render_variant_equals_the_oracle(ctx, kernel):
    """16 x 8, 3 spheres, 2 lights, 4 bounces, 2 rays per pixel, as uint64"""
    scene = edge_scene()
    want, _ = T.oracle_render(scene, 16, 8, 4, 2)
    got = T.render(ctx, scene, 16, 8, 4, 2, kernel=kernel)
    assert ctx.render_variant()["decoupled"] == (kernel == T.COMPACT)
    assert np.array_equal(bits(got), bits(want))
    assert len(np.unique(want.reshape(-1, 3), axis=0)) > 8  # more than sky
