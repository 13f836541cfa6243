"""The specular extension on the device, family by family (tests/specular_scenes.py), bit for bit against the CPU restatement
(tests/specular_restatement.c) -- which tests/test_specular_model.py holds to the oracle with the switch off and, term by term, to an
exact model of the declared rules with it on.

Every family goes through the four specular instantiations of the production kernel -- one family per sphere or one per patch of a
sphere (trt_set_path_patches 0, 2), with and without counters -- and through the reference-order kernel; render_variant() and
path_patches() say which one ran.  Each frame is 64x36 at 3 rays per pixel and 4 bounces."""
import contextlib
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import specular_scenes as SC
import specular_support as SS
import support as T
from support import bits
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S

pytestmark = pytest.mark.gpu

W, H, B, SPP = SC.W, SC.H, SC.BOUNCES, SC.SPP


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def wanted(name):
    """(scene, the restatement's frame with the switch on, its (path rays, shadow rays), the oracle's reference frame), computed once and
    read-only"""
    scene = SC.FAMILIES[name]()
    want, counts, _ = SS.render(scene, W, H, B, SPP, 1)
    plain, _ = T.oracle_render(scene, W, H, B, SPP)
    want.flags.writeable = plain.flags.writeable = False
    return scene, want, counts, plain


def lights(scene):
    return len(scene.dir_lights) + len(scene.point_lights)


@contextlib.contextmanager
def settings(ctx):
    """tables for scenes of any size; every setting back to the library's own afterwards"""
    try:
        ctx.set_kernel(hip.Context.PRODUCTION)
        ctx.set_path_grids_min_spheres(0)
        yield
    finally:
        ctx.enable_counters(False)
        ctx.set_specular(False)
        ctx.set_refraction(None)
        ctx.set_kernel(hip.Context.PRODUCTION)
        ctx.set_path_grids(64, 32)
        ctx.set_path_patches(-1)
        ctx.set_path_grids_min_spheres(12)


def tables_in_use(ctx):
    return ctx.path_patches()[1] > 0


def specular(ctx, name, m, count, what):
    """one frame of the family through the specular instantiation (patches: m > 0, counting: count); the instantiation is read back"""
    scene, want, counts, _ = wanted(name)
    ctx.set_path_patches(m)
    ctx.enable_counters(count)
    ctx.set_specular(True)
    assert ctx.specular()
    got = T.render(ctx, scene, W, H, B, SPP)
    assert ctx.path_patches()[0] == (m if tables_in_use(ctx) else 0), (what, ctx.path_patches())
    assert ctx.render_variant() == {"decoupled": False, "workgroup_threads": 256}, (what, ctx.render_variant())
    SS.same(got, want, what)
    if count:
        assert ctx.read_counters() == counts, (what, ctx.read_counters(), counts)


def reference_path_again(ctx, name):
    scene, want, _, plain = wanted(name)
    ctx.set_specular(False)
    assert not ctx.specular()
    SS.same(T.render(ctx, scene, W, H, B, SPP), plain, (name, "the extension switched off"))
    return bool((bits(want) != bits(plain)).any())


@pytest.mark.parametrize("name", list(SC.FAMILIES))
def test_every_specular_instantiation_renders_the_family(ctx, name):
    scene, want, counts, _ = wanted(name)
    with settings(ctx):
        for m in (0, 2):
            for count in (False, True):
                specular(ctx, name, m, count, (name, "patches", m, "counters", count))
        assert tables_in_use(ctx), "the families' tables, whatever the number of spheres"
        ctx.enable_counters(True)
        SS.same(T.render(ctx, scene, W, H, B, SPP, kernel=hip.Context.REFERENCE_ORDER), want, (name, "the reference-order kernel"))
        assert ctx.read_counters() == counts, (name, "the reference-order kernel", ctx.read_counters(), counts)
        assert reference_path_again(ctx, name) == (lights(scene) > 0), "the highlights change the frame of every family that has a light"


@pytest.mark.parametrize("grids", [(64, 32), (11, 3), (0, 0)], ids=["64x32", "11x3", "sweep"])
@pytest.mark.parametrize("name", ["demo", "dense"])
def test_the_table_resolution_does_not_matter(ctx, name, grids):
    with settings(ctx):
        ctx.set_path_grids(*grids)
        for m in (0, 2):
            specular(ctx, name, m, True, (name, "grids", grids, "patches", m))
        assert tables_in_use(ctx) == (grids != (0, 0))
        reference_path_again(ctx, name)


@pytest.mark.parametrize("name", ["exponents", "grazing"])
def test_aimed_rays_are_lit_as_the_restatement_lights_them(ctx, name):
    """about 2 000 rays through the production stages (with and without patches; tables and sweep) and through the reference-order
    probe: `lit` holds the clamped colour with the lights' terms, and without them once the switch is off"""
    scene = SC.FAMILIES[name]()
    rays = SC.aimed_rays(scene)
    assert 1900 <= len(rays) <= 2100
    obj, lit = SS.shade_rays(scene, rays, 1)
    _, plain = SS.shade_rays(scene, rays, 0)
    assert (obj == 1).sum() > 500 and (obj == 2).sum() > 100 and (bits(lit) != bits(plain)).any(axis=1).sum() > 1000
    with settings(ctx):
        ctx.set_specular(True)
        for m in (0, 2):
            ctx.set_path_patches(m)
            ctx.set_scene(scene)
            for families in (None, np.zeros(len(rays), dtype=np.int32)):  # the sweep; the eye's table
                got = ctx.probe_rays_production(scene.camera, rays, families)
                assert np.array_equal(got[0], obj), (name, m)
                SS.same(got[4], lit, (name, "production probe, patches", m, "tables" if families is not None else "sweep"))
        got = ctx.probe_rays(rays)
        assert np.array_equal(got[0], obj)
        SS.same(got[4], lit, (name, "reference-order probe"))
        ctx.set_specular(False)
        SS.same(ctx.probe_rays_production(scene.camera, rays)[4], plain, (name, "production probe, switched off"))
        SS.same(ctx.probe_rays(rays)[4], plain, (name, "reference-order probe, switched off"))


def test_refusals(ctx):
    scene, want, _, _ = wanted("demo")
    with settings(ctx):
        for bad in (2, -1):
            with pytest.raises(hip.TrtError) as e:
                ctx.set_specular(bad)
            assert e.value.code == -2 and "specular" in str(e.value)
        assert not ctx.specular()
        # both extensions: refused at render time, by either kernel, and the context renders again afterwards
        ctx.set_scene(scene)
        ctx.set_specular(True)
        ctx.set_refraction(np.where(np.arange(scene.num_spheres) == 0, 1.5, 0.0))
        for kernel in (hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER):
            ctx.set_kernel(kernel)
            launches = ctx.launch_count()
            with pytest.raises(hip.TrtError) as e:
                ctx.render_host(scene.camera, hip.RowSet.whole(W, H), B, SPP)
            assert e.value.code == -2 and "do not combine" in str(e.value), str(e.value)
            assert ctx.launch_count() == launches
        ctx.set_refraction(None)
        SS.same(T.render(ctx, scene, W, H, B, SPP), want, "after the refusal")
        # A scene whose image outgrows LDS: no device-image form.  The limit is the one trt_set_scene_image(ctx, 0) holds every scene to
        # -- under that setting the 1 200 spheres are refused when the scene is set, extension or not, which is shown first -- and the
        # extension holds its scenes to it under the default setting too, at render time, with a message that names it.
        big = S.synth_scene(1200, T.sky("synth"), T.bench_camera(8, 4, 2.5), seed=5)
        ctx.set_scene_image(0)
        try:
            with pytest.raises(hip.TrtError) as e:
                ctx.set_scene(big)
            assert e.value.code == -4, str(e.value)
        finally:
            ctx.set_scene_image(-1)
        ctx.set_scene(big)  # no error here
        assert ctx.render_image()["image_bytes"] > 160 * 1024
        with pytest.raises(hip.TrtError) as e:
            ctx.render_host(big.camera, hip.RowSet.whole(8, 4), 2, 1)
        assert e.value.code == -4 and "specular" in str(e.value), str(e.value)
        ctx.set_specular(False)
        got = ctx.render_host(big.camera, hip.RowSet.whole(8, 4), 2, 1)
        SS.same(got, T.oracle_render(big, 8, 4, 2, 1)[0], "the large scene with the switch off: the device image")


def test_a_batch_is_one_launch_per_camera(ctx):
    scene, want, _, _ = wanted("demo")
    cams = np.stack([scene.camera, T.bench_camera(W, H, 0.5), T.bench_camera(W, H, 10.0)])
    rows = hip.RowSet.whole(W, H)
    with settings(ctx):
        ctx.set_scene(scene)
        ctx.set_specular(True)
        got = ctx.render_host_batch(cams, rows, B, SPP)
        assert ctx.batch_info() == (3, 3), ctx.batch_info()
        SS.same(got[0], want, "the batch's first frame")
        for b, cam in enumerate(cams):
            SS.same(got[b], ctx.render_host(cam, rows, B, SPP), ("frame", b, "of the batch against a single render"))
            SS.same(got[b], SS.render(scene.with_camera(cam), W, H, B, SPP, 1)[0], ("frame", b, "of the batch against the restatement"))


def test_sharing_a_scene_leaves_the_switch_off(ctx):
    scene, want, _, plain = wanted("demo")
    with settings(ctx), hip.Context(0) as other:
        ctx.set_scene(scene)
        ctx.set_specular(True)
        other.share_scene(ctx)
        assert ctx.specular() and not other.specular()
        rows = hip.RowSet.whole(W, H)
        SS.same(other.render_host(scene.camera, rows, B, SPP), plain, "the sharer: the reference's path")
        SS.same(ctx.render_host(scene.camera, rows, B, SPP), want, "the source: still on")


CHILD = """
import sys
import numpy as np
import support as T
import specular_scenes as SC
from terminalraytracer_amd import hip
scene = SC.demo()
with hip.Context(0) as ctx:
    assert ctx.specular() == (sys.argv[1] == "1")
    ctx.set_scene(scene)
    got = ctx.render_host(scene.camera, hip.RowSet.whole(SC.W, SC.H), SC.BOUNCES, SC.SPP)
rgb = hip.render_frame_rgb8(scene, SC.W, SC.H, SC.BOUNCES, SC.SPP)
# trt_dist_* is out of scope: every frame slot's context has the extension off whatever the environment says, so that the frames of
# the slots in turn are all the reference's -- also after a caller reached a slot's context and a new scene was set
plain = T.fnv(T.oracle_render(scene, SC.W, SC.H, SC.BOUNCES, SC.SPP)[0])
with hip.Dist(0, scene, None, 0, 1, SC.W, SC.H, tile_rows=8, frames_in_flight=3) as d:
    assert [d.context(k).specular() for k in range(3)] == [False, False, False]
    assert [T.fnv(d.fetch(d.render(scene.camera, SC.BOUNCES, SC.SPP))) for _ in range(4)] == [plain] * 4
    d.context(0).set_specular(True)
    d.context(2).set_specular(True)
    d.set_scene(scene)
    assert [d.context(k).specular() for k in range(3)] == [False, False, False]
    assert [T.fnv(d.fetch(d.render(scene.camera, SC.BOUNCES, SC.SPP))) for _ in range(3)] == [plain] * 3
print(T.fnv(got), T.fnv(rgb))
"""


def test_the_default_context_and_the_environment():
    scene, want, _, plain = wanted("demo")
    lib = hip.lib()
    try:
        hip.set_default_specular(True)  # before the default context exists
        assert np.array_equal(hip.render_frame_rgb8(scene, W, H, B, SPP), T.oracle_rgb8(want))
        assert not np.array_equal(T.oracle_rgb8(want), T.oracle_rgb8(plain)), "the highlights show in the bytes"
        hip.set_default_specular(False)  # ... and on the one that exists
        assert np.array_equal(hip.render_frame_rgb8(scene, W, H, B, SPP), T.oracle_rgb8(plain))
        hip.set_default_specular(True)
        assert lib.trt_shutdown() == 0
        assert np.array_equal(hip.render_frame_rgb8(scene, W, H, B, SPP), T.oracle_rgb8(plain)), "after trt_shutdown it is off again"
        assert lib.trt_set_default_specular(2) == -2
    finally:
        lib.trt_shutdown()
    # TRT_SPECULAR in a fresh child process: the default of new contexts, the default context's too -- and not of a trt_dist's frame slots
    for value, frame in (("1", want), ("0", plain)):
        env = dict(os.environ, TRT_SPECULAR=value, PYTHONPATH=os.pathsep.join([T.ROOT, os.path.join(T.ROOT, "tests")]))
        run = subprocess.run([sys.executable, "-c", CHILD, value], capture_output=True, text=True, timeout=300, env=env, cwd=T.ROOT)
        assert run.returncode == 0, run.stderr[-800:]
        assert run.stdout.split() == [T.fnv(frame), T.fnv(T.oracle_rgb8(frame))], (value, run.stdout)


def test_a_text_kind_reads_the_same_ordered_mean(ctx):
    scene, want, _, _ = wanted("demo")
    with settings(ctx):
        ctx.set_scene(scene)
        ctx.set_specular(True)
        rows = hip.RowSet.whole(W, H)
        rgb = T.oracle_rgb8(want)
        assert np.array_equal(ctx.render_host_rgb8(scene.camera, rows, B, SPP), rgb)
        text = ctx.render_host_ansi_half(scene.camera, rows, B, SPP)
        assert np.array_equal(text, host.emitter_half_rgb8(rgb)), "the half-block text of the restatement's bytes"


def test_the_demo_program_takes_the_flag_to_the_device(tmp_path):
    """examples/trt_demo --specular --rgb8 against the same run without the flag: the same text shape, other colours"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    runs = [subprocess.run([exe, str(sky), "1", "64", "36", "--rgb8", "--step=0.04"] + flag, capture_output=True, timeout=120) for flag in ([], ["--specular"])]
    assert all(r.returncode == 0 for r in runs), [r.stderr[-300:] for r in runs]
    assert len(runs[0].stdout) == len(runs[1].stdout) > 0 and runs[0].stdout != runs[1].stdout
