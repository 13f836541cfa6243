"""The sky look-up (get_skybox_color, TRT.c:700-789) on texel, face and cube edges, held to the GENUINE reference's own answers.

tests/sky_edges.py builds, per cubemap side, directions whose texel is decided on an edge -- many of them by the rounding of one
double operation -- and tests/golden/make_golden_sky_edges.py recorded the reference's texel NUMBER for each (an index-coded sky:
tests/golden/sky_edges.npz; -1 where the reference reads outside the face and defines nothing).  Here:
  CPU  the construction is the recorded one (FNV), the oracle's look-up equals the record, the inputs cover what they claim by an
       exact rational model of the look-up, and four planted mistakes each show against the record;
  GPU  the device's FP64 form (sky_index_unit) equals the record, the FP32 estimate vouches only where it must and does where it
       can, and the kernels' fetch -- the reference-order kernel's table form and the production kernel's sky_texel_wave, whole
       waves and mixed ones -- returns the recorded texel's bytes.
Every comparison is integer or bit equality."""
import functools
import json
import os

import numpy as np
import pytest

import sky_edges as E
import support as T
from terminalraytracer_amd import hip

gpu = pytest.mark.gpu
with open(os.path.join(T.GOLDEN, "sky_edges.json")) as _fh:
    META = json.load(_fh)["sides"]
FETCH_SIDES = (3, 64, 255, 256)
SPHERE = 1


@functools.lru_cache(maxsize=None)
def recorded(dim):
    """int32 texel numbers of directions(dim): face * dim^2 + index, or -1"""
    t = np.load(os.path.join(T.GOLDEN, "sky_edges.npz"))[f"texel_{dim}"]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def oracle_numbers(dim):
    """(the oracle's number with the index clamped into the face as the library defines it, inside the face?) per direction"""
    face, index, inside = E.oracle_lookup(T.oracle(), dim, E.directions(dim)[0])
    number = face * dim * dim + np.clip(index, 0, dim * dim - 1)
    assert (inside == ((index >= 0) & (index < dim * dim))).all()
    number.setflags(write=False), inside.setflags(write=False)
    return number, inside


def decided_by_rounding(dim):
    """recorded look-ups whose index in real arithmetic is not the reference's: a condition on the inputs, from the model and the record"""
    m, want = E.model(dim), recorded(dim)
    return (want >= 0) & (m["face"] * dim * dim + m["index"] != want)


# ---- CPU -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", E.SIDES)
def test_the_construction_is_the_recorded_one(dim):
    """the directions and their numpy normalisation (TRT.c:439-450's order) have the bytes the generator saw; no build of the reference
    disagreed with the other, and nothing but texel numbers and -1 is recorded"""
    dirs, family = E.directions(dim)
    want, meta = recorded(dim), META[str(dim)]
    assert len(dirs) == len(family) == len(want) == meta["directions"]
    assert T.fnv(dirs) == meta["dirs_fnv"]
    assert T.fnv(E.normalised(dirs)) == meta["unit_fnv"]
    assert meta["builds_disagree"] == 0 and want.min() == -1 and want.max() < 6 * dim * dim
    assert int((want == -1).sum()) == meta["outside"] and int((want >= 0).sum()) == meta["recorded"]


@pytest.mark.parametrize("dim", E.SIDES)
def test_the_oracle_equals_the_reference_on_every_recorded_direction(dim):
    """trt_oracle_skybox_lookup: the recorded number wherever there is one; where the record says -1 it reports `outside`, and the
    library's clamp (past the last texel: the last texel; below zero: texel 0) brings the index into the face"""
    want = recorded(dim)
    number, inside = oracle_numbers(dim)
    assert np.array_equal(inside, want >= 0)
    assert np.array_equal(number[inside], want[inside])
    face = number // (dim * dim)
    assert ((face >= 0) & (face < 6)).all()


@pytest.mark.parametrize("dim", E.SIDES)
def test_the_double_model_equals_the_reference(dim):
    """the numpy restatement the planted mistakes are cut from is itself right: a third witness, and the mistakes' control"""
    want = recorded(dim)
    face, index = E.float_lookup(E.normalised(E.directions(dim)[0]), dim)
    assert np.array_equal((face * dim * dim + index)[want >= 0], want[want >= 0])
    assert not ((index >= 0) & (index < dim * dim))[want < 0].any()


@pytest.mark.parametrize("dim", E.SIDES)
def test_the_inputs_cover_what_they_claim(dim):
    """By the rational model, not by eye: on every face directions exactly on an edge, within 2^-40 of one, at a texel centre, and
    decided by rounding alone; from 3 texels a side up at least a tenth of the recorded look-ups are decided by rounding (the model
    and the record say so; nothing here comes from the library).  The counts are the json's."""
    m, want, meta = E.model(dim), recorded(dim), META[str(dim)]
    _, family = E.directions(dim)
    rounding = decided_by_rounding(dim)
    counts = {name: int((m["cls"] == c).sum()) for c, name in enumerate(E.CLASS_NAMES)}
    assert counts == meta["classes"] and int(rounding.sum()) == meta["decided_by_rounding"]
    assert counts["plain"] == 0
    assert ((m["cls"] == E.AT_CENTRE) == (family == E.CENTRE_FAMILY)).all()  # the construction's roles are the model's classes
    if dim >= 2:
        for face in range(6):
            on = m["face"] == face
            for cls in (E.ON_EDGE, E.NEAR_EDGE, E.AT_CENTRE):
                assert (on & (m["cls"] == cls)).any(), (dim, face, E.CLASS_NAMES[cls])
            assert (rounding & (want // (dim * dim) == face)).any(), (dim, face)
    if dim >= 3:
        share = rounding.sum() / (want >= 0).sum()
        assert share >= 0.10, (dim, share)
        assert round(float(share), 4) == meta["decided_by_rounding_share"]
    assert not rounding[m["cls"] == E.AT_CENTRE].any()


@pytest.mark.parametrize("mistake", E.MISTAKES)
def test_a_planted_mistake_shows(mistake):
    """a wrong variant of the double model disagrees with the record somewhere: the inputs tell it from the reference"""
    shown = {}
    for dim in E.SIDES:
        want = recorded(dim)
        face, index = E.float_lookup(E.normalised(E.directions(dim)[0]), dim, mistake)
        shown[dim] = int(((face * dim * dim + index)[want >= 0] != want[want >= 0]).sum())
    assert all(shown[dim] > 0 for dim in E.SIDES if dim >= 3), (mistake, shown)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("dim", E.SIDES)
def test_the_device_index_is_the_reference_s(ctx, dim):
    """sky_index_unit and sky_index_estimate (csrc/trt_device.hpp) on the normalised directions: the FP64 form gives the recorded
    number (where the reference defines none, the oracle's clamped one); the estimate equals it wherever it vouches for itself; it
    never vouches on or within 2^-40 of an edge, and always at a texel centre -- E = 2^-20 dim against an FP32 error below
    2^-21.9 dim and a centre half a texel from either edge."""
    dirs, _ = E.directions(dim)
    want, cls = recorded(dim), E.model(dim)["cls"]
    number, _ = oracle_numbers(dim)
    exact, estimate, ambiguous = ctx.selftest_sky(E.normalised(dirs), dim)
    defined = want >= 0
    differs = np.nonzero(exact[defined] != want[defined])[0]
    assert differs.size == 0, (dim, differs.size, dirs[defined][differs[:5]].tolist(), exact[defined][differs[:5]].tolist(), want[defined][differs[:5]].tolist())
    assert np.array_equal(exact[~defined], number[~defined]), dim
    sure = ambiguous == 0
    assert np.array_equal(estimate[sure], exact[sure]), (dim, int((estimate[sure] != exact[sure]).sum()))
    on_edge = (cls == E.ON_EDGE) | (cls == E.NEAR_EDGE)
    assert not sure[on_edge].any(), (dim, int(sure[on_edge].sum()), dirs[on_edge & sure][:5].tolist())
    assert sure[cls == E.AT_CENTRE].all(), (dim, int((~sure[cls == E.AT_CENTRE]).sum()), dirs[(cls == E.AT_CENTRE) & ~sure][:5].tolist())


def colour_of(number):
    """the probes' material colour of an index-coded texel: byte / 255.0 (TRT.c:866)"""
    number = np.asarray(number, dtype=np.int64)
    return np.stack([number & 255, (number >> 8) & 255, (number >> 16) & 255], axis=1) / 255.0


def sky_ray(d):
    """a ray along d that meets nothing of the demo scene: from 100 above it if it does not descend, else from 100 below the ground
    plane (y = -2), where the plane test gives t < 0"""
    return [0.0, 100.0 if d[1] >= 0 else -102.0, 0.0, d[0], d[1], d[2]]


@functools.lru_cache(maxsize=None)
def fetch_case(dim):
    """(scene, rays, expected colours): every fourth direction of each (face, class, decided by rounding?) group, at least one of each;
    the oracle's trace_ray says that each ray ends on the sky"""
    dirs, _ = E.directions(dim)
    m, want = E.model(dim), recorded(dim)
    number, _ = oracle_numbers(dim)
    group = (m["face"] * 4 + m["cls"]) * 2 + decided_by_rounding(dim)
    pick = np.sort(np.concatenate([np.nonzero(group == g)[0][::4] for g in np.unique(group)]))
    expect = np.where(want >= 0, want, number)[pick]  # outside the face: the library's definition, which the oracle states
    rays = np.array([sky_ray(d) for d in dirs[pick].tolist()])
    scene = E.coded_scene(dim)
    out = T.oracle_probe(scene, rays)
    assert (out["obj"] == T.L.NONE).all()
    assert np.array_equal(T.bits(out["material"][:, :3]), T.bits(colour_of(expect)))
    return scene, rays, colour_of(expect)


def is_sky(got, colours, tag):
    obj, _, _, material, _ = got
    assert (obj == T.L.NONE).all(), tag
    wrong = np.nonzero((T.bits(material[:, :3]) != T.bits(colours)).any(axis=1))[0]
    assert wrong.size == 0, (tag, wrong.size, wrong[:5].tolist(), (material[wrong[:5], :3] * 255.0).tolist(), (colours[wrong[:5]] * 255.0).tolist())
    assert not material[:, 3:].any(), tag


@gpu
@pytest.mark.parametrize("dim", FETCH_SIDES)
def test_the_kernels_fetch_the_recorded_texel(ctx, dim):
    """An index-coded sky over the demo spheres: the reference-order kernel (sky_texel, the table form) and the production kernel's
    stages (sky_texel_wave) return the recorded texel's bytes / 255.0 -- the face stride, the index and the 0x00BBGGRR repack, with no
    two texels alike."""
    scene, rays, colours = fetch_case(dim)
    ctx.set_scene(scene)
    is_sky(ctx.probe_rays(rays), colours, (dim, "reference-order kernel"))
    is_sky(ctx.probe_rays_production(scene.camera, rays), colours, (dim, "production stages"))


@functools.lru_cache(maxsize=None)
def wave_case():
    """(scene, rays, want): blocks of 64 rays, one wave each, side 64.  Lane roles are the construction's: a centre-family direction is
    one the estimate vouches for, an edge-family direction one it cannot.
      all 64 at texel centres: the wave stays on the estimate;
      63 centres and one edge ray in lane 0, 31 or 63: the wave takes the FP64 form, the edge lane alone selects it;
      64 edge rays;
      63 centres and an edge DIRECTION aimed at a sphere: its lane is not a sky lane, and the wave stays on the estimate."""
    dim = 64
    dirs, family = E.directions(dim)
    want = recorded(dim)
    rounding = decided_by_rounding(dim)
    up = want >= 0
    centres = np.nonzero((family == E.CENTRE_FAMILY) & up)[0]
    edges = np.nonzero((family == E.EDGE_FAMILY) & up & rounding)[0]  # the ones a wrong select would show on
    assert len(centres) >= 64 and len(edges) >= 64
    scene = E.coded_scene(dim)
    rays, numbers = [], []

    def block(lanes):
        for i in lanes:
            rays.append(sky_ray(dirs[i].tolist()))
            numbers.append(want[i])

    spread = lambda a, n, off: a[(np.arange(n) * 13 + off) % len(a)]  # noqa: E731
    block(spread(centres, 64, 0))
    for k, lane in enumerate((0, 31, 63)):
        lanes = spread(centres, 64, 5 + k).copy()
        lanes[lane] = edges[(17 * k) % len(edges)]
        block(lanes)
    block(spread(edges, 64, 3))
    lanes = spread(centres, 64, 9)
    block(lanes)
    hit_lane = len(rays) - 64 + 40
    d = dirs[edges[7]]
    centre = scene.spheres[1, :3]  # the sphere at (0, 1, 0), radius 0.5
    rays[hit_lane] = [*(centre - 5.0 * d / np.sqrt(d @ d)), *d]
    rays = np.array(rays)
    out = T.oracle_probe(scene, rays)
    sky = np.ones(len(rays), dtype=bool)
    sky[hit_lane] = False
    assert out["obj"][hit_lane] == SPHERE and (out["obj"][sky] == T.L.NONE).all()
    colours = colour_of(np.array(numbers))
    assert np.array_equal(T.bits(out["material"][sky, :3]), T.bits(colours[sky]))  # the oracle agrees with the record here too
    colours[hit_lane] = out["material"][hit_lane, :3]
    return scene, rays, sky, colours, out


@gpu
def test_mixed_waves_take_the_right_form_lane_by_lane(ctx):
    """sky_texel_wave's wave-level branch and per-lane select (csrc/trt_device.hpp), steered by the construction: see wave_case.  The
    sky lanes return the recorded texels, the lane that hits the sphere the oracle's whole answer."""
    scene, rays, sky, colours, out = wave_case()
    ctx.set_scene(scene)
    obj, point, normal, material, lit = ctx.probe_rays_production(scene.camera, rays)
    assert np.array_equal(obj, out["obj"])
    wrong = np.nonzero((T.bits(material[:, :3]) != T.bits(colours)).any(axis=1))[0]
    assert wrong.size == 0, (wrong.tolist(), (material[wrong[:5], :3] * 255.0).tolist(), (colours[wrong[:5]] * 255.0).tolist())
    hit = ~sky
    for name, got in (("point", point), ("normal", normal), ("material", material), ("lit", lit)):
        assert np.array_equal(T.bits(got[hit]), T.bits(out[name][hit])), name
