"""The specular extension on the CPU: the restatement (tests/specular_restatement.c) against the oracle with the switch off, and with it
on every logged (hit, light) term of every family (tests/specular_scenes.py) against the exact model of the declared rules
(tests/specular_model.py), bit for bit.  tests/test_specular_gpu.py then holds the device to the restatement's frames.

The model is exact arithmetic on bit patterns, so it decides every term: none is skipped.  The cap below is what a judge without exact
arithmetic would need -- a `half` whose length lies within 1e-9 relative of the 1e-4 of TRT.c:444 cannot be decided by it -- and the
families as built stay under it, which is checked from the restatement's log alone."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import exact_ieee as X
import specular_model as M
import specular_scenes as SC
import specular_support as SS
import support as T

W, H, B, SPP = SC.W, SC.H, SC.BOUNCES, SC.SPP
UNDECIDABLE_CAP = 0.01


@functools.lru_cache(maxsize=None)
def family(name):
    """(scene, frame with the switch off, frame with it on, its ray counts, its terms), computed once and read-only"""
    scene = SC.FAMILIES[name]()
    off, _, _ = SS.render(scene, W, H, B, SPP, 0)
    on, counts, terms = SS.render(scene, W, H, B, SPP, 1, log=True)
    for a in (off, on, terms):
        a.flags.writeable = False
    return scene, off, on, counts, terms


def model_term(row, normalise=True):
    p = X.patterns(row)
    spec, met = M.term(p[0:3], p[3:6], p[6:9], p[9], p[10:13], p[13], row[SS.POINT] == 1.0, normalise=normalise)
    return X.doubles(spec), met


def agrees(row, spec):
    return bool(X.same_bits(spec, row[SS.SPEC]).all())


@pytest.mark.parametrize("name", list(SC.FAMILIES))
def test_the_restatement_with_the_switch_off_is_the_oracle(name):
    scene, off, on, counts, terms = family(name)
    want, st = T.oracle_render(scene, W, H, B, SPP)
    SS.same(off, want, name)
    assert counts == (st.path_rays, st.shadow_rays), "the term changes no ray"
    lights = len(scene.dir_lights) + len(scene.point_lights)
    assert bool((T.bits(on) != T.bits(off)).any()) == (lights > 0), "the term shows in the frame of every family that has a light"
    assert len(terms) <= counts[1] and (len(terms) > 0) == (lights > 0)


@pytest.mark.parametrize("name", list(SC.FAMILIES))
def test_every_logged_term_equals_the_exact_model(name):
    _, _, _, _, terms = family(name)
    wrong = [i for i, row in enumerate(terms) if not agrees(row, model_term(row)[0])]
    assert not wrong, (name, len(wrong), "of", len(terms), terms[wrong[0]].tolist())


@pytest.mark.parametrize("name", list(SC.FAMILIES))
def test_few_terms_would_be_undecidable_without_exact_arithmetic(name):
    """from the restatement's log alone: |light_direction + view| within 1e-9 relative of 1e-4"""
    _, _, _, _, terms = family(name)
    if not len(terms):
        return
    half = terms[:, SS.LIGHT_DIR] - terms[:, SS.D]
    length = np.sqrt((half * half).sum(axis=1))
    near = np.abs(length - 1e-4) <= 1e-9 * 1e-4
    assert near.sum() <= UNDECIDABLE_CAP * len(terms), (name, int(near.sum()), len(terms))


def test_the_families_meet_what_they_were_built_for():
    _, _, _, _, terms = family("exponents")
    seen = {repr(float(e)) for e in terms[:, SS.E]}
    assert seen == {repr(float(e)) for e in SC.SPECULARITIES + (1.0, 1000.0)}, "every specularity of the wall and both ground materials are lit"
    _, _, _, _, terms = family("grazing")
    met = [model_term(row)[1] for row in terms]
    lengths = np.array([X.from_bits(m["half_length"]) for m in met])
    dots = np.array([X.from_bits(m["dot"]) for m in met])
    assert (lengths <= 1e-4).sum() >= len(SC.GRAZING_ALONG), "a half that the normalisation leaves alone, per light laid along a ray"
    assert (dots < 0.0).sum() > 100 and (dots > 1.0).sum() >= 3, "the clamp acts at both ends"
    _, _, _, _, terms = family("three and two lights")
    point = terms[terms[:, SS.POINT] == 1.0]
    assert (point[:, SS.INTENSITY] == 1.0).any() and (point[:, SS.INTENSITY] < 1.0).any(), "one light_intensity clamps, one does not"
    assert len(family("dense")[0].spheres) == 130


@pytest.mark.parametrize("n", [0, 1, 2, 3, 7, 100, 255, 1000, 65535])
def test_powi_is_within_n_roundings_of_the_exact_power(n):
    """Against the exact rational c^n, powi is within relative n * 2^-52: each of its at most 2 log2 n products adds one rounding
    (2^-53 relative) and the squarings double what is there.  Checked for results above 2^-900, where no product is denormal."""
    cs = [1.0, 0.5, 0.75, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -30, 0.999, 0.99, 0.9, 2.0 / 3.0, 0.1, 1e-3, 1.0 / 3.0, 0.3, 5e-324, 1e-160, 0.0]
    cs += [float(k) / 97.0 for k in range(1, 97)]
    cs += [1.0 - k * 7e-4 for k in range(1, 13)]  # down to 0.9916: 65535 products of them stay above 2^-900
    checked = 0
    for c in cs:
        got = X.from_bits(M.powi(X.to_bits(c), n))
        if n == 0:
            assert got == 1.0
        if c == 0.0 or (n and n * np.log2(c) < -1000.0):  # far below 2^-900: not worth a rational of millions of bits
            continue
        exact = M.exact_power(c, n)
        if exact <= Fraction(2) ** -900:
            continue
        mg, eg = X.decode(X.to_bits(got))
        error = abs(Fraction(mg) * Fraction(2) ** eg - exact)
        assert error <= exact * n * Fraction(2) ** -52, (c, n, got)
        checked += 1
    assert checked >= 10


def _view_not_negated(row):
    out = row.copy()
    out[SS.D] = -row[SS.D]
    return model_term(out)[0]


def _half_not_normalised(row):
    return model_term(row, normalise=False)[0]


def _times_the_materials_colour(row):
    spec = model_term(row)[0]
    return X.doubles([X.mul_bits(a, b) for a, b in zip(X.patterns(spec), X.patterns(row[SS.MATERIAL]))])


def _no_light_intensity(row):
    out = row.copy()
    out[SS.INTENSITY] = 1.0
    return model_term(out)[0]


def _n_rounded(row):
    out = row.copy()
    e = row[SS.E]
    if np.isfinite(e) and 0.0 <= e < 65535.0:
        out[SS.E] = np.floor(e + 0.5)
    return model_term(out)[0]


MISTAKES = {"view not negated": _view_not_negated, "half not normalised": _half_not_normalised,
            "the term multiplied by the material's colour": _times_the_materials_colour,
            "point lights without light_intensity": _no_light_intensity, "n rounded instead of truncated": _n_rounded}


@pytest.mark.parametrize("mistake", list(MISTAKES))
def test_a_planted_mistake_makes_the_model_disagree(mistake):
    """each mistake, planted in a copy of the model's inputs (or, where no input can carry it, in the model's own step), must show on
    at least one family; the sound model agrees with the same terms (test_every_logged_term_equals_the_exact_model).  Every term of a
    family is judged, in log order, up to the first that disagrees; the families are gone through up to the first that catches it."""
    caught = next((name for name in SC.FAMILIES if any(not agrees(row, MISTAKES[mistake](row)) for row in family(name)[4])), None)
    assert caught is not None, mistake
