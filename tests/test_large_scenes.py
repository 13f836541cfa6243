"""Scenes whose scene image does not fit a workgroup's LDS (trt_set_scene_image, trt_render_image): the production kernel and the
reference-order kernel read them from an image in device memory.  Frames bit for bit against the CPU oracle and the reference's
hashes, trace counts against the oracle's; scenes that fit keep the kernel they ran before."""
import os
import sys

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

sys.path.insert(0, T.GOLDEN)
import make_golden_large as G  # noqa: E402

pytestmark = pytest.mark.gpu

PRODUCTION, REFERENCE_ORDER = hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    yield
    ctx.enable_counters(False)
    ctx.set_kernel(PRODUCTION)
    ctx.set_scene_image(-1)
    ctx.set_path_patches(-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def render(ctx, scene, w, h, b, spp, kernel=PRODUCTION):
    ctx.set_kernel(kernel)
    ctx.set_scene(scene)
    return ctx.render_host(scene.camera, hip.RowSet.whole(w, h), b, spp)


def _sky():
    return T.sky("synth")


# name -> (scene, width, height, bounce limit, rays per pixel)
OVERSIZED = {
    "1500sph_96x54_b6_s4": (lambda: S.synth_scene(1500, _sky(), T.bench_camera(96, 54, 2.5), seed=5), 96, 54, 6, 4),
    "4096sph_64x36_b4_s2": (lambda: S.synth_scene(4096, _sky(), T.bench_camera(64, 36, 1.0), seed=6), 64, 36, 4, 2),
    "512sph_24dir_64x36_b4_s2": (lambda: S.synth_scene_lights(512, 24, _sky(), T.bench_camera(64, 36, 1.0), seed=7), 64, 36, 4, 2),
    # fits LDS at 64 rays per pixel; the jitter table of 2 000 pushes the image over
    "1000sph_8x4_b2_s2000": (lambda: S.synth_scene(1000, _sky(), T.bench_camera(8, 4, 1.0), seed=8), 8, 4, 2, 2000),
    # beyond the 16-bit lists of the light tables (65 535 spheres): every trace sweeps
    "66000sph_16x9_b2_s1": (lambda: S.synth_scene(66000, _sky(), T.bench_camera(16, 9, 1.0), seed=9), 16, 9, 2, 1),
}
_scenes = {}


def oversized(name):
    if name not in _scenes:
        make, w, h, b, spp = OVERSIZED[name]
        scene = make()
        want, st = T.oracle_render(scene, w, h, b, spp, threads=os.cpu_count() or 1)
        _scenes[name] = (scene, w, h, b, spp, want, (st.path_rays, st.shadow_rays))
    return _scenes[name]


@pytest.mark.parametrize("kernel", [PRODUCTION, REFERENCE_ORDER], ids=["production", "reference_order"])
@pytest.mark.parametrize("name", list(OVERSIZED))
def test_scenes_too_large_for_lds_match_the_oracle(ctx, name, kernel):
    scene, w, h, b, spp, want, counts = oversized(name)
    ctx.enable_counters(True)
    got = render(ctx, scene, w, h, b, spp, kernel)
    assert np.array_equal(bits(got), bits(want)), name
    assert ctx.read_counters() == counts
    image = ctx.render_image()
    if kernel == PRODUCTION:
        assert image["in_device_memory"], image
        assert image["image_bytes"] > 160 * 1024, image
    else:  # the reference-order kernel's records (72 B a sphere) fit LDS up to about 2 200 spheres
        assert image["in_device_memory"] == (scene.num_spheres > 2200), image


@pytest.mark.parametrize("name", ["1500sph_96x54_b6_s4", "512sph_24dir_64x36_b4_s2"])
def test_reference_order_kernel_forced_to_device_memory(ctx, name):
    scene, w, h, b, spp, want, counts = oversized(name)
    ctx.set_scene_image(1)
    ctx.enable_counters(True)
    got = render(ctx, scene, w, h, b, spp, REFERENCE_ORDER)
    assert ctx.render_image()["in_device_memory"]
    assert np.array_equal(bits(got), bits(want)), name
    assert ctx.read_counters() == counts


def test_lds_only_mode_keeps_the_capacity_errors(ctx):
    scene, w, h, b, spp, _, _ = oversized("1500sph_96x54_b6_s4")
    ctx.set_scene(scene)
    ctx.set_scene_image(0)  # a setting: the frames of the scene held fail
    with pytest.raises(hip.TrtError) as e:
        ctx.render_host(scene.camera, hip.RowSet.whole(w, h), b, spp)
    assert e.value.code == -4  # TRT_ERR_CAPACITY
    with pytest.raises(hip.TrtError) as e:
        ctx.set_scene(scene)
    assert e.value.code == -4
    scene, w, h, b, spp, _, _ = oversized("1000sph_8x4_b2_s2000")
    ctx.set_scene(scene)  # fits at 64 rays per pixel
    with pytest.raises(hip.TrtError) as e:
        ctx.render_host(scene.camera, hip.RowSet.whole(w, h), b, spp)
    assert e.value.code == -4
    ctx.set_scene_image(-1)
    got = ctx.render_host(scene.camera, hip.RowSet.whole(w, h), b, spp)
    assert np.array_equal(bits(got), bits(oversized("1000sph_8x4_b2_s2000")[5]))


def test_refraction_on_a_scene_too_large_for_lds_fails_at_render_time(ctx):
    scene, w, h, b, spp, _, _ = oversized("1500sph_96x54_b6_s4")
    ctx.set_scene(scene)  # no error here
    ctx.set_refraction(np.zeros(scene.num_spheres))
    try:
        with pytest.raises(hip.TrtError) as e:
            ctx.render_host(scene.camera, hip.RowSet.whole(w, h), b, spp)
        assert e.value.code == -4
        assert "refraction" in str(e.value)
    finally:
        ctx.set_refraction(None)


@pytest.mark.parametrize("name", sorted(G.load_cases()))
def test_reference_hashes_of_scenes_too_large_for_lds(name):
    """golden_large.json through trt_render_frame, the entry project_scene wraps (its default context, automatic mode)."""
    case = G.load_cases()[name]
    scene = G.case_scene(case)
    sc = scene.as_scene()
    screen, px = S.new_screen(case["width"], case["height"])
    import ctypes as C
    rc = hip.lib().trt_render_frame(C.byref(sc), C.byref(screen), case["bounce_limit"], case["rays_per_pixel"])
    assert rc == 0, hip.lib().trt_last_error().decode()
    assert T.fnv(px) == case["fb_fnv"]
    assert T.fnv(T.oracle_rgb8(px)) == case["rgb8_fnv"]
    assert hip.lib().trt_shutdown() == 0


@pytest.mark.parametrize("kernel", [PRODUCTION, REFERENCE_ORDER], ids=["production", "reference_order"])
@pytest.mark.parametrize("case", T.golden_cases(("small", "medium")), ids=lambda c: c["name"])
def test_device_image_renders_the_small_goldens(ctx, case, kernel):
    ctx.set_scene_image(1)
    scene = T.golden_scene(case)
    want, st = T.oracle_render(scene, case["width"], case["height"], case["bounce_limit"], case["rays_per_pixel"])
    for count in (False, True):
        ctx.enable_counters(count)
        got = render(ctx, scene, case["width"], case["height"], case["bounce_limit"], case["rays_per_pixel"], kernel)
        assert ctx.render_image()["in_device_memory"]
        assert T.fnv(got) == case["fb_fnv"]
        assert np.array_equal(bits(got), bits(want))
        if count:
            assert ctx.read_counters() == (st.path_rays, st.shadow_rays)


@pytest.mark.parametrize("n", [257, 300, 700, 1030])
def test_device_image_with_patches(ctx, n):
    scene = S.synth_scene(n, _sky(), T.bench_camera(72, 40, 2.5), seed=11)
    want, st = T.oracle_render(scene, 72, 40, 6, 4)
    ctx.set_scene_image(1)
    for m in (2, 1, 0):
        ctx.set_path_patches(m)
        for count in (False, True):
            ctx.enable_counters(count)
            got = render(ctx, scene, 72, 40, 6, 4)
            assert ctx.render_image()["in_device_memory"]
            assert np.array_equal(bits(got), bits(want)), (n, m, count)
            if count:
                assert ctx.read_counters() == (st.path_rays, st.shadow_rays)


def test_bands_on_two_lane_sets_equal_one_launch(ctx):
    """render_host renders a 1080p frame in bands on two streams, each with its own device image"""
    import torch
    scene = S.synth_scene(1500, _sky(), T.bench_camera(1920, 1080, 1.0), seed=5)
    bands = render(ctx, scene, 1920, 1080, 2, 1)
    assert ctx.render_image()["in_device_memory"]
    fb = torch.zeros(1080 * 1920 * 3, dtype=torch.float64, device="cuda:0")
    ctx.render_device(scene.camera, hip.RowSet.whole(1920, 1080), 2, 1, fb.data_ptr(), fb.numel() * 8)
    ctx.synchronize()
    assert np.array_equal(bits(bands).reshape(-1), bits(fb.cpu().numpy()))


def test_frames_in_flight_each_equal_a_frame_rendered_alone(ctx):
    import torch
    w, h = 96, 54
    scene = S.synth_scene(1500, _sky(), T.bench_camera(w, h, 1.0), seed=5)
    cams = [T.bench_camera(w, h, t) for t in (0.0, 1.0, 2.5)]
    ctx.set_scene(scene)
    alone = [ctx.render_host(c, hip.RowSet.whole(w, h), 3, 2) for c in cams]
    fbs = [torch.zeros(h * w * 3, dtype=torch.float64, device="cuda:0") for _ in cams]
    torch.cuda.synchronize()
    for c, fb in zip(cams, fbs):  # back to back, no synchronisation between them
        ctx.render_device(c, hip.RowSet.whole(w, h), 3, 2, fb.data_ptr(), fb.numel() * 8)
    ctx.synchronize()
    for a, fb in zip(alone, fbs):
        assert np.array_equal(bits(a).reshape(-1), bits(fb.cpu().numpy()))
    assert not np.array_equal(bits(alone[0]), bits(alone[1]))


def test_scenes_that_fit_keep_their_kernel(ctx):
    """automatic mode: every scene that fits keeps the LDS image and the variant, workgroups and occupancy it ran before there was a
    device image -- what LDS-only mode (the former behaviour) gives it"""
    full = T.golden_full()
    for scene, w, h, b in ((T.full_scene(full["c3_1080p_64sph_b8"]), 1920, 1080, 8),  # bench.py's frame
                           (T.full_scene(full["c5_1080p_256sph_b12_f0"]), 1920, 1080, 12),
                           (S.synth_scene(1030, _sky(), T.bench_camera(72, 40, 2.5), seed=11), 72, 40, 6)):
        seen = []
        for mode in (0, -1):
            ctx.set_scene_image(mode)
            render(ctx, scene, w, h, b, 10)
            seen.append((ctx.render_image(), ctx.render_variant(), ctx.kernel_info()))
        assert seen[0] == seen[1], (scene.num_spheres, seen)
        assert seen[1][0]["in_device_memory"] is False
        ctx.set_scene_image(1)
        render(ctx, scene, w, h, b, 10)
        assert ctx.render_image()["in_device_memory"] is True
        assert ctx.render_variant() == {"decoupled": False, "workgroup_threads": 256}
    ctx.set_scene_image(-1)
