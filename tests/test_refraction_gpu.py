"""The refraction extension on the device, family by family (tests/refraction_scenes.py), bit for bit against the oracle's restatement --
which tests/test_refraction_model.py holds to an exact model of the declared rules on the same families.

Every family goes through the four refraction instantiations of the production kernel: one family per sphere or one per patch of a
sphere (trt_set_path_patches 0, 1, 2), with and without counters; path_patches() and render_variant() say which one ran.  The lens wall
and the dolls also run at other table resolutions and on the sweep, and -- with the eye inside a refractor -- with the lean twins
forced on and off: in these a ray inside a refractor must keep its sphere's full list.  Each frame is 64x36 at 3 rays per pixel."""
import contextlib
import functools

import numpy as np
import pytest

import refraction_scenes as RS
import support as T
from support import bits
from terminalraytracer_amd import hip

pytestmark = pytest.mark.gpu

W, H, B, SPP = RS.W, RS.H, RS.BOUNCES, RS.SPP
BUILDERS = {**RS.FAMILIES, **RS.GPU_ONLY}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def wanted(name):
    """(scene, indices, the restatement's frame, its (path rays, shadow rays), the reference path's frame), computed once and read-only"""
    scene, ior = BUILDERS[name]()
    want, st = T.oracle_render_refractive(scene, ior, W, H, B, SPP)
    plain, _ = T.oracle_render(scene, W, H, B, SPP)
    want.flags.writeable = plain.flags.writeable = False
    return scene, ior, want, (st.path_rays, st.shadow_rays), plain


@contextlib.contextmanager
def settings(ctx):
    """tables for scenes of any size; every setting back to the library's own afterwards"""
    try:
        ctx.set_kernel(hip.Context.PRODUCTION)
        ctx.set_path_grids_min_spheres(0)
        yield
    finally:
        ctx.enable_counters(False)
        ctx.set_refraction(None)
        ctx.set_path_grids(64, 32)
        ctx.set_path_patches(-1)
        ctx.set_path_grids_min_spheres(12)
        ctx.set_path_lean_lists(-1)


def same(got, want, what):
    """as test_degenerate_scenes_match_the_oracle compares frames that may hold values that are not finite: NaNs in the same places (x86-64
    and the GPU make different NaNs), every other value -- the infinite ones too -- bit for bit"""
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaNs in other places", int((np.isnan(got) != np.isnan(want)).sum()))
    there = ~np.isnan(want)
    differ = bits(got)[there] != bits(want)[there]
    assert not differ.any(), (what, "values differ", int(differ.sum()), np.argwhere(bits(got) != bits(want))[:4].tolist())


def tables_in_use(ctx):
    return ctx.path_patches()[1] > 0  # patches per sphere (one without patches); none: every path ray sweeps


def refract(ctx, name, m, count, what):
    """one frame of the family through the refraction instantiation (patches: m > 0, counting: count); the instantiation is read back"""
    scene, ior, want, counts, _ = wanted(name)
    ctx.set_path_patches(m)
    ctx.enable_counters(count)
    ctx.set_refraction(ior)
    got = T.render(ctx, scene, W, H, B, SPP)
    assert ctx.path_patches()[0] == (m if tables_in_use(ctx) else 0), (what, ctx.path_patches())  # trt_get_path_patches: the kernel has patches when this is > 0
    assert ctx.render_variant() == {"decoupled": False, "workgroup_threads": 256}, (what, ctx.render_variant())
    same(got, want, what)
    if count:
        assert ctx.read_counters() == counts, (what, ctx.read_counters(), counts)


def reference_path_again(ctx, name):
    scene, _, want, _, plain = wanted(name)
    ctx.set_refraction(None)
    same(T.render(ctx, scene, W, H, B, SPP), plain, (name, "the extension switched off"))
    return bool((bits(want) != bits(plain)).any())


@pytest.mark.parametrize("name", list(BUILDERS))
def test_every_refraction_instantiation_renders_the_family(ctx, name):
    with settings(ctx):
        for m in (0, 1, 2):
            for count in (False, True):
                refract(ctx, name, m, count, (name, "patches", m, "counters", count))
        assert tables_in_use(ctx), "the families' tables, whatever the number of spheres"
        assert reference_path_again(ctx, name), "the refractors change the frame"


@pytest.mark.parametrize("grids", [(64, 32), (11, 3), (0, 0)], ids=["64x32", "11x3", "sweep"])
@pytest.mark.parametrize("name", ["lens wall", "dolls"])
def test_the_table_resolution_does_not_matter(ctx, name, grids):
    with settings(ctx):
        ctx.set_path_grids(*grids)
        for m in (0, 2):
            refract(ctx, name, m, True, (name, "grids", grids, "patches", m))
        assert tables_in_use(ctx) == (grids != (0, 0))
        reference_path_again(ctx, name)


@pytest.mark.parametrize("lean", [1, 0], ids=["lean twins", "full lists"])
@pytest.mark.parametrize("name", ["lens wall", "dolls", "eye inside"])
def test_a_ray_inside_a_refractor_keeps_the_full_list(ctx, name, lean):
    with settings(ctx):
        ctx.set_path_lean_lists(lean)
        for m in (0, 1):
            refract(ctx, name, m, True, (name, "lean lists", lean, "patches", m))
            assert ctx.path_lean_lists()["in_use"] == bool(lean), (name, lean, m)
        reference_path_again(ctx, name)


def test_index_edge_values_outside_the_domain_are_refused(ctx):
    """NaN, +inf, -1.5 and 1e200 on the lens wall: trt_set_refraction takes 0 <= ior < 1e6 and refuses these, one by one and together, with
    TRT_ERR_ARGUMENT; the values it takes -- 1e-200, a denormal, 1.0 and the doubles either side of it -- render like any family
    (test_every_refraction_instantiation_renders_the_family[index edges])"""
    scene, edges = RS.index_edges()
    _, ior, want, _, _ = wanted("index edges")
    refused = [v for v in RS.EDGE_INDICES if not RS.index_accepted(v)]
    assert len(refused) == 4 and len(ior) == len(edges)
    with settings(ctx):
        ctx.set_scene(scene)
        for bad in [edges] + [np.where(np.arange(len(ior)) == 3 * k, v, ior) for k, v in enumerate(refused)]:
            with pytest.raises(hip.TrtError) as e:
                ctx.set_refraction(bad)
            assert e.value.code == -2 and "index of refraction" in str(e.value), str(e.value)
        ctx.set_refraction(ior)
        same(T.render(ctx, scene, W, H, B, SPP), want, "the accepted values after the refused ones")
