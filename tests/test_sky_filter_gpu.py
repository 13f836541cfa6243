"""Bilinear sky filtering on the device, family by family and sky by sky (tests/sky_filter_support.py), bit for bit against the CPU
restatement (tests/sky_filter_restatement.c) -- which tests/test_sky_filter_model.py holds to the oracle with the switch off and, look-up
by look-up, to an exact model of the declared rules with it on.

Every case goes through the four filtering instantiations of the production kernel -- one family per sphere or one per patch of a
sphere (trt_set_path_patches 0, 2), with and without counters -- and through the reference-order kernel; render_variant() and
path_patches() say which one ran.  Each frame is 64x36 at 3 rays per pixel and 4 bounces."""
import contextlib
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import sky_edges as E
import sky_filter_support as SF
import support as T
from support import bits
from terminalraytracer_amd import hip

pytestmark = pytest.mark.gpu

W, H, B, SPP = SF.W, SF.H, SF.BOUNCES, SF.SPP
SKIES = ("1", "2", "3", "64", "colors256")  # small sides: every weight non-trivial, face edges in most pixels; one 256^2 sky of the fixtures
CASES = [(family, sky) for family in SF.FAMILIES for sky in SKIES] + [("demo", "checker256")]  # ... whose faces are not of one colour
PROBE_SIDES = (1, 2, 3, 64, 256, 2048)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def wanted(family, sky):
    """(scene, the restatement's frame with the filter on, its (path rays, shadow rays), the oracle's reference frame and its counts),
    computed once and read-only"""
    scene = SF.FAMILIES[family](SF.SKIES[sky]())
    want, counts, _ = SF.render(scene, 1)
    plain, st = T.oracle_render(scene, W, H, B, SPP)
    want.flags.writeable = plain.flags.writeable = False
    return scene, want, counts, plain, (st.path_rays, st.shadow_rays)


@contextlib.contextmanager
def settings(ctx):
    """tables for scenes of any size; every setting back to the library's own afterwards"""
    try:
        ctx.set_kernel(hip.Context.PRODUCTION)
        ctx.set_path_grids_min_spheres(0)
        yield
    finally:
        ctx.enable_counters(False)
        ctx.set_sky_filter(hip.SKY_NEAREST)
        ctx.set_specular(False)
        ctx.set_refraction(None)
        ctx.set_scene_image(-1)
        ctx.set_kernel(hip.Context.PRODUCTION)
        ctx.set_path_patches(-1)
        ctx.set_path_grids_min_spheres(12)


def tables_in_use(ctx):
    return ctx.path_patches()[1] > 0


def filtered(ctx, family, sky, m, count, what):
    """one frame of the case through the filtering instantiation (patches: m > 0, counting: count); the instantiation is read back"""
    scene, want, counts, _, oracle_counts = wanted(family, sky)
    ctx.set_path_patches(m)
    ctx.enable_counters(count)
    ctx.set_sky_filter(hip.SKY_BILINEAR)
    assert ctx.sky_filter() == hip.SKY_BILINEAR
    got = T.render(ctx, scene, W, H, B, SPP)
    assert ctx.path_patches()[0] == (m if tables_in_use(ctx) else 0), (what, ctx.path_patches())
    assert ctx.render_variant() == {"decoupled": False, "workgroup_threads": 256}, (what, ctx.render_variant())
    SF.same(got, want, what)
    if count:
        assert ctx.read_counters() == oracle_counts == counts, (what, ctx.read_counters(), oracle_counts)


@pytest.mark.parametrize("family,sky", CASES)
def test_every_filtering_instantiation_renders_the_case(ctx, family, sky):
    scene, want, counts, plain, oracle_counts = wanted(family, sky)
    with settings(ctx):
        for m in (0, 2):
            for count in (False, True):
                filtered(ctx, family, sky, m, count, (family, sky, "patches", m, "counters", count))
        assert tables_in_use(ctx), "the families' tables, whatever the number of spheres -- none included"
        ctx.enable_counters(True)
        SF.same(T.render(ctx, scene, W, H, B, SPP, kernel=hip.Context.REFERENCE_ORDER), want, (family, sky, "the reference-order kernel"))
        assert ctx.read_counters() == oracle_counts, (family, sky, "the reference-order kernel", ctx.read_counters())
        ctx.set_scene_image(1)  # ... and its form that reads the scene's records from device memory
        SF.same(T.render(ctx, scene, W, H, B, SPP, kernel=hip.Context.REFERENCE_ORDER), want, (family, sky, "the reference-order kernel, device scene"))
        ctx.set_scene_image(-1)
        # switched off again: the oracle's frame on the same context
        ctx.set_sky_filter(hip.SKY_NEAREST)
        assert ctx.sky_filter() == hip.SKY_NEAREST
        SF.same(T.render(ctx, scene, W, H, B, SPP), plain, (family, sky, "the filter switched off"))
        assert bool((bits(want) != bits(plain)).any()) == (sky not in SF.UNIFORM), "the filter shows under every sky whose faces are not of one colour"


@functools.lru_cache(maxsize=None)
def probe_case(dim):
    """(scene, rays, what the restatement says each meets, its material): the edge directions of the side and directions that are not
    numbers, from a point above a scene with no sphere and a ground no ray meets"""
    dirs = np.concatenate([E.directions(dim)[0], SF.SHORT_NUMBERS, SF.NOT_NUMBERS, np.zeros((1, 3))])
    rays = np.concatenate([np.broadcast_to(np.array([0.0, 1.0, 0.0]), dirs.shape), dirs], axis=1)
    scene = SF.sky_only(SF.hashed_sky(dim))
    obj, material = SF.shade_rays(scene, rays, 1)
    assert not obj.any(), "every ray ends on the sky"
    _, nearest = SF.shade_rays(scene, rays, 0)
    assert dim == 1 or (bits(material[:, :3]) != bits(nearest[:, :3])).any(axis=1).sum() > len(rays) // 4, "the blend differs from the nearest texel"
    return scene, rays, material


@pytest.mark.parametrize("dim", PROBE_SIDES)
def test_single_rays_take_the_restatement_s_colour(ctx, dim):
    """trt_probe_rays and trt_probe_rays_production with the filter on: the material colour of a miss is the blend, bit for bit, on texel
    edges +-3 ulps, face edges, cube corners, lattice points and centres at three scales, and for directions that are not numbers;
    reflectivity and specularity of the miss stay 0"""
    scene, rays, material = probe_case(dim)
    with settings(ctx):
        ctx.set_scene(scene)
        ctx.set_sky_filter(hip.SKY_BILINEAR)
        for name, got in (("reference-order probe", ctx.probe_rays(rays)), ("production stages", ctx.probe_rays_production(scene.camera, rays))):
            assert not got[0].any(), (dim, name)
            wrong = np.nonzero((bits(got[3]) != bits(material)).any(axis=1))[0]
            assert wrong.size == 0, (dim, name, wrong.size, wrong[:5].tolist(), rays[wrong[:5], 3:].tolist(), got[3][wrong[:5]].tolist(), material[wrong[:5]].tolist())


def test_other_output_kinds_and_a_batch_read_the_same_ordered_mean(ctx):
    scene, want, _, _, _ = wanted("mirrors", "3")
    cams = np.stack([scene.camera, T.bench_camera(W, H, 0.5), T.bench_camera(W, H, 10.0)])
    rows = hip.RowSet.whole(W, H)
    with settings(ctx):
        ctx.set_scene(scene)
        ctx.set_sky_filter(hip.SKY_BILINEAR)
        assert np.array_equal(ctx.render_host_rgb8(scene.camera, rows, B, SPP), T.oracle_rgb8(want))
        got = ctx.render_host_batch(cams, rows, B, SPP)  # trt_render_device_batch behind it: one launch per camera
        assert ctx.batch_info() == (3, 3), ctx.batch_info()
        SF.same(got[0], want, "the batch's first frame")
        for b, cam in enumerate(cams):
            SF.same(got[b], ctx.render_host(cam, rows, B, SPP), ("frame", b, "of the batch against a single render"))
            SF.same(got[b], SF.render(scene.with_camera(cam), 1)[0], ("frame", b, "of the batch against the restatement"))


def test_refusals(ctx):
    scene, want, _, _, _ = wanted("demo", "64")
    rows = hip.RowSet.whole(W, H)
    with settings(ctx):
        for bad in (2, -1):
            with pytest.raises(hip.TrtError) as e:
                ctx.set_sky_filter(bad)
            assert e.value.code == -2 and "sky filter" in str(e.value)
        assert ctx.sky_filter() == hip.SKY_NEAREST
        ctx.set_scene(scene)
        ctx.set_sky_filter(hip.SKY_BILINEAR)
        # with another extension: refused at render time, by either kernel, with a message that names both switches
        for other, switch_on, switch_off in (("trt_set_refraction", lambda: ctx.set_refraction(np.where(np.arange(scene.num_spheres) == 0, 1.5, 0.0)), lambda: ctx.set_refraction(None)),
                                             ("trt_set_specular", lambda: ctx.set_specular(True), lambda: ctx.set_specular(False))):
            switch_on()
            for kernel in (hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER):
                ctx.set_kernel(kernel)
                launches = ctx.launch_count()
                with pytest.raises(hip.TrtError) as e:
                    ctx.render_host(scene.camera, rows, B, SPP)
                assert e.value.code == -2 and "trt_set_sky_filter" in str(e.value) and other in str(e.value), str(e.value)
                assert ctx.launch_count() == launches
            switch_off()
            ctx.set_kernel(hip.Context.PRODUCTION)
        SF.same(T.render(ctx, scene, W, H, B, SPP), want, "after the refusals")
        # the device image: the filtering instantiations have none
        ctx.set_scene_image(1)
        launches = ctx.launch_count()
        with pytest.raises(hip.TrtError) as e:
            ctx.render_host(scene.camera, rows, B, SPP)
        assert e.value.code == -4 and "sky filtering" in str(e.value), str(e.value)
        assert ctx.launch_count() == launches
        ctx.set_scene_image(-1)
        SF.same(ctx.render_host(scene.camera, rows, B, SPP), want, "after the refusal")


def test_sharing_a_scene_leaves_the_filter_off(ctx):
    scene, want, _, plain, _ = wanted("demo", "64")
    with settings(ctx), hip.Context(0) as other:
        ctx.set_scene(scene)
        ctx.set_sky_filter(hip.SKY_BILINEAR)
        other.set_sky_filter(hip.SKY_BILINEAR)
        other.share_scene(ctx)
        assert ctx.sky_filter() == hip.SKY_BILINEAR and other.sky_filter() == hip.SKY_NEAREST
        rows = hip.RowSet.whole(W, H)
        SF.same(other.render_host(scene.camera, rows, B, SPP), plain, "the sharer: the reference's path")
        SF.same(ctx.render_host(scene.camera, rows, B, SPP), want, "the source: still on")


CHILD = """
import sys
import support as T
import sky_filter_support as SF
from terminalraytracer_amd import hip
scene = SF.demo(SF.hashed_sky(64))
with hip.Context(0) as ctx:
    assert ctx.sky_filter() == int(sys.argv[1])
    ctx.set_scene(scene)
    got = ctx.render_host(scene.camera, hip.RowSet.whole(SF.W, SF.H), SF.BOUNCES, SF.SPP)
rgb = hip.render_frame_rgb8(scene, SF.W, SF.H, SF.BOUNCES, SF.SPP)
# every frame slot of a trt_dist has the filter off whatever the environment says -- also after a caller reached a slot's context and
# a new scene was set
plain = T.fnv(T.oracle_render(scene, SF.W, SF.H, SF.BOUNCES, SF.SPP)[0])
with hip.Dist(0, scene, None, 0, 1, SF.W, SF.H, tile_rows=8, frames_in_flight=3) as d:
    assert [d.context(k).sky_filter() for k in range(3)] == [0, 0, 0]
    assert [T.fnv(d.fetch(d.render(scene.camera, SF.BOUNCES, SF.SPP))) for _ in range(4)] == [plain] * 4
    d.context(0).set_sky_filter(1)
    d.context(2).set_sky_filter(1)
    d.set_scene(scene)
    assert [d.context(k).sky_filter() for k in range(3)] == [0, 0, 0]
    assert [T.fnv(d.fetch(d.render(scene.camera, SF.BOUNCES, SF.SPP))) for _ in range(3)] == [plain] * 3
print(T.fnv(got), T.fnv(rgb))
"""


def test_the_default_context_and_the_environment():
    scene, want, _, plain, _ = wanted("demo", "64")
    lib = hip.lib()
    try:
        hip.set_default_sky_filter(hip.SKY_BILINEAR)  # before the default context exists
        assert np.array_equal(hip.render_frame_rgb8(scene, W, H, B, SPP), T.oracle_rgb8(want))
        assert not np.array_equal(T.oracle_rgb8(want), T.oracle_rgb8(plain)), "the filter shows in the bytes"
        hip.set_default_sky_filter(hip.SKY_NEAREST)  # ... and on the one that exists
        assert np.array_equal(hip.render_frame_rgb8(scene, W, H, B, SPP), T.oracle_rgb8(plain))
        hip.set_default_sky_filter(hip.SKY_BILINEAR)
        assert lib.trt_shutdown() == 0
        assert np.array_equal(hip.render_frame_rgb8(scene, W, H, B, SPP), T.oracle_rgb8(plain)), "after trt_shutdown it is off again"
        assert lib.trt_set_default_sky_filter(2) == -2
        # the drop-in entry itself, void project_scene(Scene *, Screen *) at its 10 bounces and 10 rays per pixel
        assert lib.trt_shutdown() == 0
        hip.set_default_sky_filter(hip.SKY_BILINEAR)
        SF.same(hip.project_scene(scene, W, H), SF.render(scene, 1, shot=(10, 10))[0], "project_scene behind trt_set_default_sky_filter")
        hip.set_default_sky_filter(hip.SKY_NEAREST)
        SF.same(hip.project_scene(scene, W, H), T.oracle_render(scene, W, H, 10, 10)[0], "project_scene with the filter off again")
    finally:
        lib.trt_shutdown()
    # TRT_SKY_FILTER in a fresh child process: the default of new contexts, the default context's too -- and not of a trt_dist's frame slots
    for value, frame in (("1", want), ("0", plain)):
        env = dict(os.environ, TRT_SKY_FILTER=value, PYTHONPATH=os.pathsep.join([T.ROOT, os.path.join(T.ROOT, "tests")]))
        run = subprocess.run([sys.executable, "-c", CHILD, value], capture_output=True, text=True, timeout=300, env=env, cwd=T.ROOT)
        assert run.returncode == 0, run.stderr[-800:]
        assert run.stdout.split() == [T.fnv(frame), T.fnv(T.oracle_rgb8(frame))], (value, run.stdout)


def test_the_demo_program_takes_the_flag_to_the_device(tmp_path):
    """examples/trt_demo --sky-filter --rgb8 against the same run without the flag: the same text shape, other colours"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "uv_checker"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("uv_checker", f))
    runs = [subprocess.run([exe, str(sky), "1", "64", "36", "--rgb8", "--step=0.04"] + flag, capture_output=True, timeout=120) for flag in ([], ["--sky-filter"])]
    assert all(r.returncode == 0 for r in runs), [r.stderr[-300:] for r in runs]
    assert len(runs[0].stdout) == len(runs[1].stdout) > 0 and runs[0].stdout != runs[1].stdout
