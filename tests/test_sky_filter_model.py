"""Bilinear sky filtering on the CPU: the restatement (tests/sky_filter_restatement.c) against the oracle with the switch off, and with it
on every logged look-up -- of rendered frames and of the edge directions of tests/sky_edges.py -- against the exact model of the
declared rules (tests/sky_filter_model.py), bit for bit: the face, the four taps, the two weights, the texels and the colour.
tests/test_sky_filter_gpu.py then holds the device to the restatement.

Facts the lerp form was chosen for (include/trt_hip.h): (a) four equal taps give byte / 255.0; (b) fx = fy = 0 gives the texel
(i0, j0); (c) a channel never leaves the range of its four taps."""
import functools

import numpy as np
import pytest

import exact_ieee as X
import sky_edges as E
import sky_filter_model as M
import sky_filter_support as SF
import support as T

# every family under a small and a large sky; every sky under some family
FRAMES = [("demo", "1"), ("demo", "64"), ("demo", "colors256"), ("mirrors", "2"), ("mirrors", "3"), ("mirrors", "synth64"),
          ("no sphere", "3"), ("no sphere", "64"), ("fourteen spheres", "2"), ("fourteen spheres", "checker256")]
SIDES = (1, 2, 3, 5, 64, 256, 2048)


@functools.lru_cache(maxsize=None)
def frame(family, sky):
    """(scene, frame with the switch off, frame with it on, its ray counts, its look-ups), computed once and read-only"""
    scene = SF.FAMILIES[family](SF.SKIES[sky]())
    off, _, _ = SF.render(scene, 0)
    on, counts, looks = SF.render(scene, 1, log=True)
    for a in (off, on, looks):
        a.flags.writeable = False
    return scene, off, on, counts, looks


def disagreement(row, sky):
    """None if the model's look-up of the row's direction is the row, else what differs first"""
    m = M.lookup(X.patterns(row[SF.DIRECTION]), sky)
    if (m["face"],) + m["taps"] != tuple(int(v) for v in row[SF.FACE:SF.J1 + 1]):
        return "face or taps", (m["face"],) + m["taps"]
    if [m["fx"], m["fy"]] != X.patterns(row[SF.FX:SF.FY + 1]):
        return "weights", X.doubles([m["fx"], m["fy"]]).tolist()
    if [r + 256 * g + 65536 * b for r, g, b in m["texels"]] != [int(v) for v in row[SF.TAPS]]:
        return "texels", m["texels"]
    if m["colour"] != X.patterns(row[SF.COLOUR]):
        return "colour", X.doubles(m["colour"]).tolist()
    return None


def first_disagreement(looks, sky):
    return next(((i, d) for i, d in ((i, disagreement(row, sky)) for i, row in enumerate(looks)) if d is not None), None)


@functools.lru_cache(maxsize=None)
def edge_looks(dim):
    dirs, family = E.directions(dim)
    dirs = np.concatenate([dirs, SF.SHORT_NUMBERS, SF.NOT_NUMBERS, np.zeros((1, 3))])
    looks = SF.lookups(SF.hashed_sky(dim), dirs)
    looks.flags.writeable = False
    return looks, family


@pytest.mark.parametrize("family,sky", FRAMES)
def test_the_restatement_with_the_switch_off_is_the_oracle(family, sky):
    scene, off, on, counts, looks = frame(family, sky)
    want, st = T.oracle_render(scene, SF.W, SF.H, SF.BOUNCES, SF.SPP)
    SF.same(off, want, (family, sky))
    assert counts == (st.path_rays, st.shadow_rays), "the filter changes no ray"
    assert 0 < len(looks) <= SF.W * SF.H * SF.SPP
    assert bool((T.bits(on) != T.bits(off)).any()) == (sky not in SF.UNIFORM), "the filter shows in every frame whose faces are not of one colour"


@pytest.mark.parametrize("family,sky", FRAMES)
def test_every_look_up_of_a_frame_equals_the_exact_model(family, sky):
    scene, _, _, _, looks = frame(family, sky)
    assert first_disagreement(looks, scene.sky) is None, (family, sky, len(looks))


@pytest.mark.parametrize("dim", SIDES)
def test_every_edge_direction_equals_the_exact_model(dim):
    """texel edges +-3 ulps, face edges, cube corners, lattice points, centres, at scales 0.3 / 1 / 7; directions that are not numbers,
    vectors so short that the scaling overflows, and vectors just long enough that it does not"""
    looks, _ = edge_looks(dim)
    assert first_disagreement(looks, SF.hashed_sky(dim)) is None, dim
    odd = looks[-len(SF.NOT_NUMBERS) - 1:]
    assert not odd[:, SF.FACE:SF.FY + 1].any(), "face 0, four times texel 0, both weights 0"
    first = SF.hashed_sky(dim)[0, 0, 0] / 255.0
    assert (T.bits(odd[:, SF.COLOUR]) == T.bits(first)).all(), "the colour the nearest look-up defines for them"
    short = looks[-len(SF.NOT_NUMBERS) - 1 - len(SF.SHORT_NUMBERS):-len(SF.NOT_NUMBERS) - 1]
    assert short[:, SF.FACE].tolist() == [0.0, 1.0, 0.0] and (dim == 1 or short[:, SF.FX:SF.FY + 1].any()), "numbers like any other"


def test_four_equal_taps_give_the_reference_s_value():
    """(a) under six uniform faces the frame with the switch on is the oracle's frame"""
    for family in SF.FAMILIES:
        scene = SF.FAMILIES[family](SF.uniform_sky())
        on, _, looks = SF.render(scene, 1, log=True)
        assert len(looks) and (looks[:, SF.FX] > 0).any() and (looks[:, SF.FY] > 0).any()
        SF.same(on, T.oracle_render(scene, SF.W, SF.H, SF.BOUNCES, SF.SPP)[0], family)


@pytest.mark.parametrize("dim", SIDES)
def test_zero_weights_give_the_texel_itself(dim):
    """(b) on the `centre` family: where both weights are 0 the colour is the texel (i0, j0) over 255 exactly, and at a texel's centre
    that is the texel the nearest look-up returns"""
    looks, family = edge_looks(dim)
    dirs, _ = E.directions(dim)
    centre = np.nonzero(family == E.CENTRE_FAMILY)[0]
    sky = SF.hashed_sky(dim)
    exact = centre[(looks[centre, SF.FX] == 0.0) & (looks[centre, SF.FY] == 0.0)]
    assert len(exact) >= 6, (dim, len(exact), len(centre))
    rows = looks[exact]
    texel = sky[rows[:, SF.FACE].astype(int), rows[:, SF.J0].astype(int), rows[:, SF.I0].astype(int)]
    assert np.array_equal(T.bits(rows[:, SF.COLOUR]), T.bits(texel / 255.0))
    face, index = E.float_lookup(E.normalised(dirs[exact]), dim)
    assert np.array_equal(face, rows[:, SF.FACE].astype(int)) and np.array_equal(index, (rows[:, SF.I0] + rows[:, SF.J0] * dim).astype(int))
    # the other centres: within an ulp or so of one, so the weights are next to 0 or to 1 and the colour within 1e-9 of a texel's
    near = looks[centre]
    w = np.minimum(near[:, [SF.FX, SF.FY]], 1.0 - near[:, [SF.FX, SF.FY]])
    assert (w < 1e-9).all(), (dim, float(w.max()))


def within_its_taps(looks):
    taps = looks[:, SF.TAPS].astype(np.int64)
    for c in range(3):
        channel = ((taps >> (8 * c)) & 255) / 255.0
        value = looks[:, SF.COLOUR][:, c]
        if not ((channel.min(axis=1) <= value) & (value <= channel.max(axis=1))).all():
            return False
    return True


def test_no_channel_leaves_the_range_of_its_taps():
    """(c), over every look-up of every frame and of every edge family"""
    for family, sky in FRAMES:
        assert within_its_taps(frame(family, sky)[4]), (family, sky)
    for dim in SIDES:
        looks, _ = edge_looks(dim)
        assert within_its_taps(looks), dim
        assert (looks[:, [SF.FX, SF.FY]] >= 0.0).all() and (looks[:, [SF.FX, SF.FY]] < 1.0).all()


@pytest.mark.parametrize("mistake", list(SF.MISTAKES))
def test_a_planted_mistake_is_caught(mistake):
    """the restatement with one wrong step (its `mistake` argument) logs a look-up the model disagrees with, in the frames of some
    family or in some side's edge directions; the sound restatement's look-ups all agree (the tests above)"""
    number = SF.MISTAKES[mistake]

    def caught():
        for family, sky in (("mirrors", "3"), ("demo", "64")):
            scene = SF.FAMILIES[family](SF.SKIES[sky]())
            if first_disagreement(SF.render(scene, 1, log=True, mistake=number)[2], scene.sky) is not None:
                yield family, sky
        for dim in (3, 5):
            if first_disagreement(SF.lookups(SF.hashed_sky(dim), E.directions(dim)[0], mistake=number), SF.hashed_sky(dim)) is not None:
                yield "edges", dim

    assert next(caught(), None) is not None, mistake
