"""Several cameras of one scene per call (trt_render_device_batch, trt_render_host_batch, trt_batch_info): where the production
kernel has a BATCH form, ONE persistent launch works through the samples of all the frames.  Every frame of a batch must be,
bit for bit, what trt_render_device gives for that camera -- and so what the CPU oracle and the reference give."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import support as T
from support import anim_cameras
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

gpu = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4


# ---- without a GPU ----

def test_the_batch_entries_are_declared_exported_and_bound():
    header = open(os.path.join(T.ROOT, "include", "trt_hip.h")).read()
    dll = hip.lib()
    for name in ("trt_render_device_batch", "trt_render_host_batch", "trt_batch_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/trt_hip.h"
        assert hasattr(dll, name), name + " is not exported"
        assert name in hip.SYMBOLS
    for method in ("render_device_batch", "render_host_batch", "batch_info"):
        assert callable(getattr(hip.Context, method))


def test_batch_max_is_the_number_of_eye_slots():
    header = open(os.path.join(T.ROOT, "include", "trt_hip.h")).read()
    csrc = os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")
    assert int(re.search(r"#define\s+TRT_BATCH_MAX\s+(\d+)", header).group(1)) == 8
    assert int(re.search(r"constexpr int kEyeSlots = (\d+);", open(os.path.join(csrc, "trt_context.hpp")).read()).group(1)) == 8
    assert re.search(r"static_assert\(TRT_BATCH_MAX == kEyeSlots", open(os.path.join(csrc, "trt_render.hip")).read())


def test_refusals_that_need_no_device():
    """NULL arguments are refused before anything touches the GPU"""
    lib = hip.lib()
    rows = hip.RowSet.whole(8, 4)
    assert lib.trt_render_device_batch(None, None, 1, C.byref(rows), 4, 1, None, 0) == ARGUMENT
    assert lib.trt_render_host_batch(None, None, 1, C.byref(rows), 4, 1, None) == ARGUMENT
    assert lib.trt_batch_info(None, None, None) == ARGUMENT


# ---- fuzzed batches: the cases are plain data, made without a GPU ----

FUZZ_SEEDS = tuple(range(12)) + (13, 24, 29, 44)  # 24 and 44: no lights; 29: no spheres
FUZZ_TINY = (6, 13)  # seeds whose frames have fewer samples than a wave: one wave holds samples of several frames
FUZZ_TABLES = (((0, 0), -1, -1), ((64, 32), 2, -1), ((64, 32), -1, 0), ((64, 32), -1, 1))  # path grids, patches, compaction
FUZZ_NAN = (1, 3, 9, 10)  # seeds whose every fourth sphere has a colour that is not a number: the cameras that see one have NaN pixels


@functools.lru_cache(maxsize=None)
def fuzz_batch_case(seed):
    """(scene, cameras[n, 15], w, h, bounce limit, rays per pixel) of a fuzzed batch: a fuzz scene seen by 1 to 8 cameras of one screen whose
    eyes are drawn independently -- on the orbit, inside sphere 0, far away, on a point light, or the eye of ANOTHER camera of the
    batch with another basis (the two legitimately share one eye-table key).  No finite camera makes the oracle's frame non-finite
    (a NaN or infinite one sends the reference's own sky look-up out of its cubemap), so the NaN frames come from a material: in the
    seeds of FUZZ_NAN every fourth sphere's colour is NaN, which reaches pixels through the shading arithmetic alone, never through geometry."""
    rng = np.random.default_rng(2000 + seed)
    w, h = int(rng.integers(8, 72)), int(rng.integers(4, 40))
    b, spp = int(rng.integers(1, 9)), int(rng.choice([1, 3, 10]))
    if seed in FUZZ_TINY:
        w, h, spp = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.choice([1, 2]))
        assert w * h * spp < 64
    scene = T.fuzz_scene(rng, w, h)
    if seed in FUZZ_NAN:
        spheres = scene.spheres.copy()
        spheres[::4, 4:7] = np.nan
        scene = scene.with_spheres(spheres)
    n = int(rng.integers(1, 9))
    cams = np.zeros((n, 15))
    for k in range(n):
        cams[k] = T.bench_camera(w, h, float(rng.choice([0.0, 0.5, 1.0, 2.5, 10.0, 33.3])))  # an orbit camera: its basis, eye and the batch's screen
        kind = rng.choice(["orbit", "inside", "far", "same eye", "on a light"], p=[0.4, 0.15, 0.15, 0.25, 0.05])
        if kind == "inside" and scene.num_spheres:
            cams[k, 9:12] = scene.spheres[0, :3] + 0.3 * scene.spheres[0, 3]
        elif kind == "far":
            cams[k, 9:12] = rng.normal(size=3) * 20
        elif kind == "same eye" and k:
            cams[k, 9:12] = cams[int(rng.integers(0, k)), 9:12]
        elif kind == "on a light" and scene.point_lights.shape[0]:
            cams[k, 9:12] = scene.point_lights[0, :3]
    if seed % 4 == 0:
        cams[0] = scene.camera  # the camera the fuzz scene came with
    return scene, cams, w, h, b, spp


@functools.lru_cache(maxsize=None)
def fuzz_batch_oracle(seed, k):
    scene, cams, w, h, b, spp = fuzz_batch_case(seed)
    with np.errstate(all="ignore"):
        return T.oracle_render(scene.with_camera(cams[k]), w, h, b, spp)[0]


def test_fuzzed_batch_cases_are_mostly_finite():
    """Where the oracle's frame has NaNs the fuzz compares their positions and the finite values only; that branch hides little only
    if it is rare: at most one case (camera x seed) in eight takes it, by the oracle alone.  And the cases are what they claim."""
    assert len(FUZZ_SEEDS) >= 16
    cases, nans, same_eye, lights = 0, 0, 0, set()
    for seed in FUZZ_SEEDS:
        scene, cams, w, h, b, spp = fuzz_batch_case(seed)
        assert 1 <= len(cams) <= 8 and (cams[:, 12:15] == cams[0, 12:15]).all()
        assert (w * h * spp < 64) == (seed in FUZZ_TINY)
        lights.add(scene.dir_lights.shape[0] + scene.point_lights.shape[0])
        eyes = [tuple(c[9:12]) for c in cams]
        same_eye += sum(1 for k in range(len(cams)) for j in range(k) if eyes[j] == eyes[k] and not np.array_equal(cams[j, :9], cams[k, :9]))
        for k in range(len(cams)):
            cases += 1
            nans += not np.isfinite(fuzz_batch_oracle(seed, k)).all()
    print(f"{nans} of {cases} fuzzed batch frames are not finite")
    assert nans >= 1 and nans * 8 <= cases, (nans, cases)
    for seed in FUZZ_SEEDS:  # compaction 1 (the decoupled BATCH form) on scenes of two or more lights
        if FUZZ_TABLES[seed % 4][2] == 1:
            scene = fuzz_batch_case(seed)[0]
            assert scene.dir_lights.shape[0] + scene.point_lights.shape[0] >= 2, seed
    spheres = {fuzz_batch_case(s)[0].num_spheres for s in FUZZ_SEEDS}
    assert same_eye >= 3 and 0 in lights and max(lights) >= 4 and 0 in spheres and len(spheres) >= 5
    assert any(len(fuzz_batch_case(s)[1]) == 1 for s in FUZZ_SEEDS) and any(len(fuzz_batch_case(s)[1]) == 8 for s in FUZZ_SEEDS)


# ---- on the GPU ----

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
        c.set_kernel(hip.Context.PRODUCTION)
        c.set_refraction(None)
        c.set_path_grids(64, 32)
        c.set_path_patches(-1)
        c.set_path_grids_min_spheres(12)
        c.set_compaction(-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def frame_rows(rows):
    lib = hip.lib()
    return [lib.trt_rowset_frame_row(C.byref(rows), i) for i in range(lib.trt_rowset_rows(C.byref(rows)))]


@functools.lru_cache(maxsize=None)
def _scene(kind):
    cam = anim_cameras([0], 160, 48)[0]
    return S.demo_scene(T.sky("synth"), cam) if kind == "demo" else S.synth_scene(64, T.sky("synth"), cam)


@functools.lru_cache(maxsize=None)
def _oracle(kind, w, h, index, b, spp):
    scene = _scene(kind).with_camera(anim_cameras([index], w, h)[0])
    return T.oracle_render(scene, w, h, b, spp)[0]


def check_batch(ctx, kind, w, h, indices, b, spp, rows=None, launches=1, oracle=True):
    """one batch of the cameras `indices`: every frame == the oracle's rows == render_host for that camera"""
    rows = rows or hip.RowSet.whole(w, h)
    cams = anim_cameras(indices, w, h)
    got = ctx.render_host_batch(cams, rows, b, spp)
    assert ctx.batch_info() == (len(indices), launches if launches else len(indices))
    owned = frame_rows(rows)
    assert got.shape == (len(indices), len(owned), w, 3)
    for k, index in enumerate(indices):
        single = ctx.render_host(cams[k], rows, b, spp)
        assert np.array_equal(bits(got[k]), bits(single)), f"frame {k} (camera {index}) differs from the single call"
        if oracle:
            want = _oracle(kind, w, h, index, b, spp)[owned]
            assert np.array_equal(bits(got[k]), bits(want)), f"frame {k} (camera {index}) differs from the oracle"
    return got


FULL = {"c3": ["c3_1080p_64sph_b8_f0", "c3_1080p_64sph_b8_f19", "c3_1080p_64sph_b8_f59"],
        "c5": ["c5_1080p_256sph_b12_f0", "c5_1080p_256sph_b12_f59"]}


@gpu
@pytest.mark.parametrize("config", sorted(FULL))
def test_full_size_batches_reproduce_the_reference_hashes_from_one_launch(ctx, config):
    """BASELINE configs 3 and 5 at 1920x1080, the cameras the reference's hashes were recorded for, one batch each: every frame's
    FNV is the reference's, from ONE render launch; config 3 (64 spheres, no patches, a large launch) runs the decoupled BATCH
    form (128 VGPRs, no scratch, 4 waves per SIMD: profiles/r07/a_batch.md)."""
    import torch
    cases = [T.golden_full()[name] for name in FULL[config]]
    c0 = cases[0]
    w, h, n = c0["width"], c0["height"], len(cases)
    ctx.set_scene(T.full_scene(c0))
    cams = np.array([c["camera"] for c in cases], dtype=np.float64)
    fb = torch.zeros(n * h * w * 3, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device_batch(cams, hip.RowSet.whole(w, h), c0["bounce_limit"], c0["rays_per_pixel"], fb.data_ptr(), fb.numel() * 8)
    ctx.synchronize()
    assert ctx.batch_info() == (n, 1)
    if config == "c3":
        assert ctx.render_variant()["decoupled"]
    frames = fb.cpu().numpy().reshape(n, h, w, 3)
    for k, case in enumerate(cases):
        assert T.fnv(frames[k]) == case["fb_fnv"], case["name"]
    assert len(ctx.kernel_times(4)) >= 1


@gpu
@pytest.mark.parametrize("kind,w,h", [("demo", 160, 48), ("demo", 67, 13), ("synth", 160, 48), ("synth", 67, 13)])
def test_small_batches_equal_the_oracle_and_single_calls(ctx, kind, w, h):
    ctx.set_scene(_scene(kind))
    picks = {1: [12], 2: [3, 41], 3: [0, 19, 59], 8: [0, 7, 15, 22, 30, 37, 45, 59]}
    for n, indices in picks.items():
        for spp in (1, 3, 10):
            check_batch(ctx, kind, w, h, indices, 4, spp)
            check_batch(ctx, kind, w, h, indices, 4, spp, rows=hip.RowSet.shard(w, h, 1, 3, 4))
    check_batch(ctx, kind, w, h, [5, 5], 4, 3)          # the same camera twice
    check_batch(ctx, kind, w, h, [0, 30, 0], 6, 3)      # opposite sides of the orbit: the cameras look away from each other


@gpu
def test_table_settings_keep_the_frames_and_the_single_launch(ctx):
    w, h, indices = 96, 54, [0, 19, 37, 59]
    for grids, patches, compaction in (((0, 0), -1, -1), ((64, 32), 2, -1), ((64, 32), -1, 0), ((64, 32), -1, 1)):
        ctx.set_path_grids(*grids)
        ctx.set_path_patches(patches)
        ctx.set_compaction(compaction)
        ctx.set_scene(_scene("synth"))
        check_batch(ctx, "synth", w, h, indices, 5, 4)
        if compaction == 1:
            assert ctx.render_variant()["decoupled"]
        if patches == 2:
            assert ctx.path_patches()[0] == 2


@gpu
def test_what_has_no_batch_form_is_served_per_camera(ctx):
    w, h, indices = 64, 36, [0, 19, 59]
    cams = anim_cameras(indices, w, h)
    rows = hip.RowSet.whole(w, h)
    scene = _scene("synth")
    # counters: cleared once per batch, the batch's totals
    ctx.set_scene(scene)
    ctx.enable_counters(True)
    singles = []
    for cam in cams:
        ctx.render_host(cam, rows, 5, 3)
        singles.append(ctx.read_counters())
    check_batch(ctx, "synth", w, h, indices, 5, 3, launches=0)
    ctx.render_host_batch(cams, rows, 5, 3)
    assert ctx.read_counters() == tuple(sum(s[i] for s in singles) for i in (0, 1))
    ctx.enable_counters(False)
    # the reference-order kernel
    ctx.set_kernel(hip.Context.REFERENCE_ORDER)
    check_batch(ctx, "synth", w, h, indices, 5, 3, launches=0)
    ctx.set_kernel(hip.Context.PRODUCTION)
    # the refraction extension, against its CPU restatement
    small = S.synth_scene(24, T.sky("synth"), cams[0], seed=3)
    ior = np.where(np.arange(24) % 3 == 0, 1.5, 0.0)
    ctx.set_scene(small)
    ctx.set_refraction(ior)
    got = ctx.render_host_batch(cams, rows, 6, 2)
    assert ctx.batch_info() == (3, 3)
    for k, cam in enumerate(cams):
        want, _ = T.oracle_render_refractive(small.with_camera(cam), ior, w, h, 6, 2)
        assert np.array_equal(bits(got[k]), bits(want))
    ctx.set_refraction(None)
    # a scene whose image does not fit LDS
    big = S.synth_scene(1500, T.sky("synth"), cams[0], seed=5)
    ctx.set_scene(big)
    got = ctx.render_host_batch(cams, rows, 4, 1)
    assert ctx.batch_info() == (3, 3) and ctx.render_image()["in_device_memory"]
    for k, cam in enumerate(cams):
        assert np.array_equal(bits(got[k]), bits(ctx.render_host(cam, rows, 4, 1)))
    ctx.set_scene(scene)  # a small scene again before the fixture restores the table settings


@gpu
def test_batches_and_single_frames_interleave_on_one_context(ctx):
    """queue hand-over between launches of different shapes, and the eye-slot caches: a single frame after a batch must not
    trust a slot the batch overwrote, nor a batch a slot of the batch before it"""
    ctx.set_scene(_scene("synth"))
    wa, ha, wb, hb = 160, 48, 67, 13
    cam_a, cam_b = anim_cameras([7], wa, ha)[0], anim_cameras([44], wb, hb)[0]
    want_a, want_b = _oracle("synth", wa, ha, 7, 4, 3), _oracle("synth", wb, hb, 44, 4, 10)
    assert np.array_equal(bits(ctx.render_host(cam_a, hip.RowSet.whole(wa, ha), 4, 3)), bits(want_a))
    check_batch(ctx, "synth", wa, ha, [21, 7, 33], 4, 3)
    assert np.array_equal(bits(ctx.render_host(cam_b, hip.RowSet.whole(wb, hb), 4, 10)), bits(want_b))
    check_batch(ctx, "synth", wa, ha, [33, 21], 4, 3, rows=hip.RowSet.shard(wa, ha, 1, 3, 4))
    assert np.array_equal(bits(ctx.render_host(cam_a, hip.RowSet.whole(wa, ha), 4, 3)), bits(want_a))
    # the batch's frames straight after one another, without single frames between them that would rebuild slot 0
    cams = anim_cameras([7, 21, 33], wa, ha)
    first = ctx.render_host_batch(cams, hip.RowSet.whole(wa, ha), 4, 3)
    again = ctx.render_host_batch(cams[::-1].copy(), hip.RowSet.whole(wa, ha), 4, 3)
    assert np.array_equal(bits(first), bits(again[::-1]))
    assert np.array_equal(bits(first[0]), bits(want_a))


@gpu
def test_refusals_leave_the_context_rendering(ctx):
    import torch
    w, h = 67, 13
    scene = _scene("synth")
    rows = hip.RowSet.whole(w, h)
    cams = anim_cameras([0, 19], w, h)
    with hip.Context(0) as empty:
        with pytest.raises(hip.TrtError) as e:
            empty.render_host_batch(cams, rows, 4, 1)
        assert e.value.code == NO_SCENE
    ctx.set_scene(scene)

    def refused(code, cameras, capacity=None):
        fb = torch.zeros(2 * h * w * 3, dtype=torch.float64, device="cuda:0")
        with pytest.raises(hip.TrtError) as e:
            ctx.render_device_batch(cameras, rows, 4, 1, fb.data_ptr(), fb.numel() * 8 if capacity is None else capacity)
        assert e.value.code == code, e.value
        ctx.synchronize()

    refused(ARGUMENT, np.zeros((0, 15)))
    refused(ARGUMENT, anim_cameras(range(9), w, h))
    other = cams.copy()
    other[1, 13] *= 2
    refused(ARGUMENT, other)
    refused(CAPACITY, cams, capacity=2 * h * w * 24 - 8)
    with hip.Context(0) as sharer:
        sharer.share_scene(ctx)
        refused(CAPACITY, cams)
        assert "shared" in hip.lib().trt_last_error().decode()
        with pytest.raises(hip.TrtError) as e:
            sharer.render_host_batch(cams, rows, 4, 1)
        assert e.value.code == CAPACITY
        one = sharer.render_host_batch(cams[:1], rows, 4, 1)  # one camera always works
        assert np.array_equal(bits(one[0]), bits(_oracle("synth", w, h, 0, 4, 1)))
    assert np.array_equal(bits(ctx.render_host(cams[1], rows, 4, 1)), bits(_oracle("synth", w, h, 19, 4, 1)))
    check_batch(ctx, "synth", w, h, [0, 19], 4, 1)


@gpu
def test_a_batch_whose_image_would_cost_a_workgroup_is_split(ctx):
    """Near 290 spheres the image of ONE frame still fits a CU's LDS four times and the image of eight frames (224 B per extra
    camera, 136 B per sphere) no longer does: somewhere in this range of sphere counts a batch of 8 is cut into several launches
    (the largest parts that keep the occupancy); split or not, every frame is the single call's."""
    w, h = 32, 18
    rows = hip.RowSet.whole(w, h)
    cams = anim_cameras([0, 7, 15, 22, 30, 37, 45, 59], w, h)
    ctx.set_path_patches(0)
    launches = {}
    for spheres in range(276, 300, 2):
        ctx.set_scene(S.synth_scene(spheres, T.sky("synth"), cams[0], seed=17))
        got = ctx.render_host_batch(cams, rows, 4, 2)
        launches[spheres] = ctx.batch_info()[1]
        for k, cam in enumerate(cams):
            assert np.array_equal(bits(got[k]), bits(ctx.render_host(cam, rows, 4, 2))), (spheres, k)
    ctx.set_scene(_scene("synth"))
    print("render launches of a batch of 8 by sphere count:", launches)
    assert any(1 < n for n in launches.values()), launches
    assert any(n == 1 for n in launches.values()), launches


@gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS, ids=[f"seed{s}" for s in FUZZ_SEEDS])
def test_fuzzed_batches_match_the_oracle(ctx, seed):
    """Batches of anything but the demo and SYNTH scenes seen from the orbit: no spheres, no lights, many lights, duplicated, nested
    and zero-radius spheres, tilted and non-unit ground normals, cameras inside a sphere, far away, on a light, two cameras of one
    eye -- under the table settings of test_table_settings_keep_the_frames_and_the_single_launch, with the path tables for scenes of
    any size on every other seed.  Every frame is the oracle's and the single call's."""
    scene, cams, w, h, b, spp = fuzz_batch_case(seed)
    grids, patches, compaction = FUZZ_TABLES[seed % 4]
    rows = hip.RowSet.whole(w, h)
    ctx.set_path_grids(*grids)
    ctx.set_path_patches(patches)
    ctx.set_compaction(compaction)
    ctx.set_path_grids_min_spheres(0 if seed % 2 else 12)
    ctx.set_scene(scene)
    got = ctx.render_host_batch(cams, rows, b, spp)
    frames, launches = ctx.batch_info()
    assert frames == len(cams) and 1 <= launches <= len(cams)
    for k, cam in enumerate(cams):
        want = fuzz_batch_oracle(seed, k)
        single = ctx.render_host(cam, rows, b, spp)
        finite = np.isfinite(want)
        print(f"seed {seed} camera {k}: {w}x{h} b={b} spp={spp}, {scene.num_spheres} spheres, {int((~finite).sum())} non-finite values")
        if finite.all():
            assert np.array_equal(bits(got[k]), bits(want)), (seed, k)
            assert np.array_equal(bits(got[k]), bits(single)), (seed, k)
        else:  # as test_fuzzed_scenes_match_the_oracle: the NaNs in the same places, the finite values bit-equal
            for frame in (got[k], single):
                assert np.array_equal(np.isnan(frame), np.isnan(want)) and np.array_equal(bits(frame[finite]), bits(want[finite])), (seed, k)
    ctx.set_scene(_scene("synth"))  # a scene the restored table settings build quickly for


@gpu
def test_the_frame_index_packed_beside_the_bounce_count(ctx):
    """A BATCH launch keeps the frame's index in the three bits of the bounce count above kBatchBounceMask = 2^28 - 1 and masks on
    every compare: the largest limit it takes must leave those bits alone (one launch, the oracle's frames), and one more must send
    the call to the per-camera path (three launches, the same bits)."""
    w, h, spp, indices = 32, 18, 2, [0, 19, 59]
    cams = anim_cameras(indices, w, h)
    spheres = S.synth_spheres(64)
    spheres[:, 7] = np.minimum(spheres[:, 7], 0.9)
    scene = S.synth_scene(64, T.sky("synth"), cams[0]).with_spheres(spheres)
    # the guard, before anything is launched: nothing reflects more than 0.9, so every path ends by the reference's weight > 0.00001
    # cut (0.9^110 < 0.00001) within 110 bounces whatever the limit -- a perfect mirror would keep a persistent kernel spinning
    assert (scene.spheres[:, 7] <= 0.9).all() and scene.ground[9] <= 0.9 and scene.ground[14] <= 0.9
    assert 0.9 ** 110 < 0.00001
    mask = 2 ** 28 - 1
    want = [T.oracle_render(scene.with_camera(cam), w, h, mask, spp)[0] for cam in cams]
    for k, cam in enumerate(cams):  # the oracle at that limit is the oracle at any limit above the longest path
        assert np.array_equal(bits(want[k]), bits(T.oracle_render(scene.with_camera(cam), w, h, 111, spp)[0]))
        assert np.isfinite(want[k]).all()
    rows = hip.RowSet.whole(w, h)
    ctx.set_scene(scene)
    assert ctx.read_path_tables(cams[0])[0]["enabled"]
    got = ctx.render_host_batch(cams, rows, mask, spp)
    assert ctx.batch_info() == (3, 1)
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    again = ctx.render_host_batch(cams, rows, mask + 1, spp)
    assert ctx.batch_info() == (3, 3)
    assert np.array_equal(bits(again), bits(got))
