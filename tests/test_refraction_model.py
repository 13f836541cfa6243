"""The refraction extension held to an exact model, bend by bend (CPU only).

The extension's only judge used to be oracle/trt_oracle.c's shade_pixel_refractive, which was written from the kernel: a mistake both
share -- an inverted eta, a normal that faces the wrong way on leaving, a nudge to the wrong side -- passed every test.  Here the
restatement renders each scene family of tests/refraction_scenes.py once, single-threaded, logging its path rays, and
tests/refraction_model.py -- 60-digit decimal arithmetic, written from the declared rules (include/trt_hip.h, trt_set_refraction) and the
textbook form of Snell's law -- predicts every next ray from the logged one, and the number of path rays of every sample.  The device is
then held to the restatement bit for bit on the same families (tests/test_refraction_gpu.py).

Tolerance: 1e-10 absolute per component, between restatement and model (never the kernel).  A semantic error moves an origin by at
least the 1e-6 nudge or a direction by far more; rounding moves them by 1e-12.  Largest deviations measured with these scenes:

    family        origin    direction  declined / events
    lens wall     1.3e-13   4.3e-13    11 / 16245
    dolls         5.7e-13   2.9e-13     0 / 19283
    eye inside    5.7e-13   6.5e-14     0 / 13792
    grazing 1.5   1.0e-13   6.0e-14     0 / 18449
    grazing 0.7   1.0e-13   9.6e-14     0 / 14257
    floor         6.9e-14   5.1e-13     0 / 15922
    old scene     9.9e-13   1.4e-12     1 / 41862

The two largest are the old 24-sphere frame's: the direction after an "enter" whose sphere had disc / b^2 = 2.5e-6, just above the
model's 1e-6 exclusion, and an origin on the ground."""
import functools

import numpy as np
import pytest

import refraction_model as M
import refraction_scenes as RS
import support as T

TOLERANCE = 1e-10


@functools.lru_cache(maxsize=None)
def logged(name):
    """(scene, indices, stats, path rays) of the family's frame, rendered once"""
    scene, ior = RS.FAMILIES[name]()
    w, h, b, spp = RS.MODEL_SHOT[name]
    _, st, rays = T.oracle_path_rays_refractive(scene, ior, w, h, b, spp)
    rays.flags.writeable = False
    return scene, ior, st, rays


@functools.lru_cache(maxsize=None)
def judged(name):
    scene, ior, _, rays = logged(name)
    return M.check_frame(scene, ior, rays, RS.MODEL_SHOT[name][2], TOLERANCE)


def test_the_builders_are_deterministic():
    for name, build in {**RS.FAMILIES, **RS.GPU_ONLY}.items():
        (a, ia), (b, ib) = build(), build()
        for x, y in ((a.spheres, b.spheres), (a.ground, b.ground), (a.dir_lights, b.dir_lights), (a.point_lights, b.point_lights), (a.camera, b.camera), (ia, ib)):
            assert np.array_equal(T.bits(x), T.bits(y)), name
        assert len(ia) == a.num_spheres, name
    scene, ior = RS.index_edges()
    assert np.isnan(ior[0]) and ior[1] == np.inf and ior[5] == 5e-324 and ior[7] < 1.0 < ior[8], "the edge values reach the scene as they are"
    assert np.array_equal(T.bits(scene.spheres), T.bits(RS.lens_wall()[0].spheres))
    assert [v for v in RS.EDGE_INDICES if RS.index_accepted(v)] == [1e-200, 5e-324, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)]
    assert set(RS.index_edges_accepted()[1]) == {1e-200, 5e-324, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 0.0}


@pytest.mark.parametrize("name", list(RS.FAMILIES))
def test_the_restatement_agrees_with_the_exact_model(name):
    """every sample is logged; every sample the model did not decline logs as many path rays as the model predicts; every judged event
    agrees within the tolerance; the model declines at most 1 % of the events"""
    scene, ior, st, rays = logged(name)
    w, h, b, spp = RS.MODEL_SHOT[name]
    got = judged(name)
    print(name, {k: v for k, v in got.items() if k != "classes"}, got["classes"])
    assert len(rays) == st.path_rays
    assert got["samples"] == w * h * spp == st.samples
    assert got["wrong lengths"] == 0, got["first"]
    assert got["wrong rays"] == 0, got["first"]
    assert max(got["origin"], got["direction"]) <= TOLERANCE
    assert got["declined"] * 100 <= got["events"], (got["declined"], got["events"])
    assert max(got["origin"], got["direction"]) <= 1e-11, ("a conditioning the exclusions miss?", got["worst"])


# judged events per family and class, written out: what the families must reach.  Order of a row: M.CLASSES
COVERAGE = {
    "lens wall": (1387, 557, 1350, 384, 199, 279, 136, 5041),
    "dolls": (1910, 2297, 1908, 0, 0, 0, 620, 5636),
    "eye inside": (615, 11, 615, 0, 0, 0, 0, 5639),
    "grazing 1.5": (3024, 0, 3022, 40, 0, 3049, 1, 2401),
    "grazing 0.7": (19, 0, 19, 0, 3025, 16, 1, 4265),
    "floor": (907, 0, 892, 207, 0, 58, 4, 6942),
    "old scene": (766, 0, 762, 27, 19, 8, 6, 19538),
}
OWN_CLASS = {"lens wall": ("enter while inside another", "total reflection inside", "opaque sphere while inside"), "dolls": ("enter while inside another", "opaque sphere while inside"),
             "eye inside": ("enter", "enter while inside another"), "grazing 1.5": ("enter", "ground while inside"), "grazing 0.7": ("total reflection from outside",),
             "floor": ("ground while inside", "total reflection inside"), "old scene": ("total reflection inside", "total reflection from outside")}


def test_the_families_cover_every_event_class():
    found = {name: tuple(judged(name)["classes"][c] for c in M.CLASSES) for name in RS.FAMILIES}
    for name, row in found.items():
        print(f'    "{name}": {row},')
    assert found == COVERAGE
    for k, c in enumerate(M.CLASSES):
        assert sum(row[k] for row in found.values()) >= 100, c
    for name, classes in OWN_CLASS.items():  # each family sees its own classes
        for c in classes:
            assert found[name][M.CLASSES.index(c)] >= 10, (name, c)


# the family on which each planted mistake must show
PLANTED = {"eta inverted": "lens wall", "normal not flipped on leaving": "lens wall", "refracted origin at p + back": "grazing 1.5",
           "near root inside": "dolls", "outer refractor remembered": "dolls"}


@pytest.mark.parametrize("mistake", M.MISTAKES)
def test_the_model_can_fail(mistake):
    """the same logs, the model with one deliberate mistake: it must report disagreement (and none without the mistake)"""
    name = PLANTED[mistake]
    scene, ior, _, rays = logged(name)
    right = judged(name)
    assert right["wrong rays"] == 0 and right["wrong lengths"] == 0
    got = M.check_frame(scene, ior, rays, RS.MODEL_SHOT[name][2], TOLERANCE, mistake=mistake, stop_after=50)
    print(mistake, got["wrong rays"], got["wrong lengths"], got["first"])
    assert got["wrong rays"] + got["wrong lengths"] >= 50, (mistake, got["first"])
