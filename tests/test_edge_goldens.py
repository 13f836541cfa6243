"""The adversarial scene families against the reference's OWN frames (tests/golden/edges.npz, golden_edges.json, recorded by
tests/golden/make_golden_edges.py from the compiled reference): the degenerate scenes, the fuzz seeds and the blocker-distance lights
that the oracle alone used to judge, and the value-domain scenes -- reflectivities at the END-round threshold, above one, negative,
infinite, NaN, huge; light and sphere colours and intensities out of every sane range; eyes so far out that the checker's (int)
conversion leaves `int` -- which nothing judged.

The oracle and the kernels were restated by one hand from one reading of TRT.c; here each answers to the reference itself.  A frame
equals the record when its NaNs sit in the same places (their signs and payloads are the machine's: x86-64 and the GPU make different
default NaNs), every other value has the same bits, the counts of NaN and infinite values are the recorded ones and the FNV of the
frame with its NaNs made one NaN is the recorded hash.  Where the archive keeps a case's hash only, the positions of a difference come
from the oracle's frame, which the CPU test of the same case pins to that hash."""
import functools

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import hip
from support import KERNEL_IDS, KERNELS, bits, render

gpu = pytest.mark.gpu
CASES = T.edge_cases()
IDS = [c["name"] for c in CASES]
NON_FINITE = [c for c in CASES if T.must_hold_nans(c["name"], c["b"])]
MAX_NAN_SHARE = 0.10


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """(frame, stats) of the oracle for a case: rendered once, shared by the tests, never written to"""
    case = next(c for c in CASES if c["name"] == name)
    with np.errstate(all="ignore"):
        px, st = T.oracle_render(T.edge_scene(case), case["w"], case["h"], case["b"], case["spp"])
    px.flags.writeable = False
    return px, st


def assert_is_the_recorded_frame(got, case, positions_from, who):
    """`positions_from`: the frame that says where the NaNs and the values are -- the record where the archive holds it, else the oracle's"""
    T.assert_is_the_recorded_frame(got, case, T.edge_fb(case), positions_from, who)


# ---- CPU: the fixture is what it claims, and the oracle equals it ----

def test_the_record_covers_every_family_and_hides_little():
    """The conditions make_golden_edges.py writes under: a case's NaNs are at most a tenth of its values, so that a failure cannot hide
    among them, and the scenes named for non-finite inputs do have NaNs (from the bounce limit at which their values reach the frame),
    so that the non-finite path really runs."""
    assert {c["family"] for c in CASES} == {"degenerate", "fuzz", "blocker", "values"}
    assert "No case was dropped" in T.edge_meta()["note"]
    assert len(NON_FINITE) >= 6 and {c["name"].split("/")[1] for c in NON_FINITE} == set(T.NON_FINITE_VALUES)
    for c in CASES:
        assert c["nan"] <= MAX_NAN_SHARE * c["w"] * c["h"] * 3, c["name"]
        assert c["w"] <= 96 and c["h"] <= 54
        if c in NON_FINITE:
            assert c["nan"] > 0, c["name"]
        fb = T.edge_fb(c)
        if fb is not None:
            assert (int(np.isnan(fb).sum()), int(np.isinf(fb).sum())) == (c["nan"], c["inf"]) and T.fnv(T.canonical_nans(fb)) == c["fb_fnv"], c["name"]


def test_the_builders_still_make_the_recorded_scenes():
    """test_gpu_parity.py renders these scenes from their builders (tests/support.py) and judges them by the oracle; the record was
    made from the same builders.  Bit for bit, NaNs and signed zeros included, so the two sets of tests are about the same inputs."""
    built = T.edge_case_inputs()
    assert [(n, f, k, w, h, b, s) for n, f, k, _, w, h, b, s in built] == [(c["name"], c["family"], c["scene"], c["w"], c["h"], c["b"], c["spp"]) for c in CASES]
    for (name, _, _, scene, *_), case in zip(built, CASES):
        assert np.array_equal(bits(T.pack_scene(scene)), bits(T.pack_scene(T.edge_scene(case)))), name


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_equals_the_reference_frame(case):
    px, st = oracle_frame(case["name"])
    assert_is_the_recorded_frame(px, case, px, "oracle")
    assert st.samples == case["w"] * case["h"] * case["spp"]


def test_a_light_direction_that_is_not_a_number_counts_as_full_light():
    """T.non_finite_light_scene: fmin(NaN, 1.0) is 1.0, so the oracle's frame holds no NaN; with a min that passes a NaN on, every
    lit pixel would be one.  The reference is not defined on this scene (see the builder), so the oracle judges the kernels below."""
    for b, spp in T.VALUE_SHOTS:
        with np.errstate(all="ignore"):
            px, st = T.oracle_render(T.non_finite_light_scene(), *T.VALUE_SIZE, b, spp)
        assert np.isfinite(px).all() and px.max() <= 1.0 and px.min() >= 0.0
        assert st.shadow_rays >= 4 * T.VALUE_SIZE[0] * T.VALUE_SIZE[1] * spp // 2  # four lights per hit, most first rays hit


# ---- GPU ----

@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.set_path_grids_min_spheres(0)
    c.set_scratch_fill(True)  # a unit a launch drops reads as a NaN the reference does not have: it cannot hide among those it does have
    yield c
    c.close()


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_kernel_equals_the_reference_frame(ctx, case):
    """The production kernel as it ships, with the decoupling forced and the reference-order kernel, then the production kernel
    reading the scene from device memory (the DEVICE_IMAGE instantiations); the trace counts are the oracle's."""
    scene, (want, st) = T.edge_scene(case), oracle_frame(case["name"])
    w, h, b, spp = case["w"], case["h"], case["b"], case["spp"]
    ctx.enable_counters(True)
    try:
        for kernel, who in list(zip(KERNELS, KERNEL_IDS)) + [(hip.Context.PRODUCTION, "production_rounds, device image")]:
            in_device_memory = who.endswith("device image")
            ctx.set_scene_image(1 if in_device_memory else -1)
            got = render(ctx, scene, w, h, b, spp, kernel)
            if in_device_memory:
                assert ctx.render_image()["in_device_memory"], who
            assert_is_the_recorded_frame(got, case, want, who)
            assert ctx.read_counters() == (st.path_rays, st.shadow_rays), (case["name"], who)
    finally:
        ctx.enable_counters(False)
        ctx.set_scene_image(-1)


@gpu
@pytest.mark.parametrize("b,spp", T.VALUE_SHOTS)
def test_a_light_direction_that_is_not_a_number_on_the_device(ctx, b, spp):
    """min1 (fmin(n.l, 1.0), NaN -> 1.0) with the only NaN operand it can get: every kernel and the device-image form against the
    oracle, bit for bit and finite, with its counts.  The scratch fill is on: a NaN here is a dropped unit or a min that lets it pass."""
    scene = T.non_finite_light_scene()
    w, h = T.VALUE_SIZE
    with np.errstate(all="ignore"):
        want, st = T.oracle_render(scene, w, h, b, spp)
    assert np.isfinite(want).all()
    ctx.enable_counters(True)
    try:
        for kernel, who in list(zip(KERNELS, KERNEL_IDS)) + [(hip.Context.PRODUCTION, "production_rounds, device image")]:
            ctx.set_scene_image(1 if who.endswith("device image") else -1)
            got = render(ctx, scene, w, h, b, spp, kernel)
            assert np.array_equal(bits(got), bits(want)), (who, int(np.isnan(got).sum()), int((bits(got) != bits(want)).sum()))
            assert ctx.read_counters() == (st.path_rays, st.shadow_rays), who
    finally:
        ctx.enable_counters(False)
        ctx.set_scene_image(-1)


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_batch_holds_the_reference_frame_twice(ctx, case):
    """trt_render_device_batch with the case's camera, another stored camera, and the case's camera again: the first and the last
    frame are the recorded one, the one between them is the oracle's for that camera."""
    import torch
    scene, (want, _) = T.edge_scene(case), oracle_frame(case["name"])
    w, h, b, spp = case["w"], case["h"], case["b"], case["spp"]
    other = T.bench_camera(w, h, 10.0)
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_compaction(-1)
    ctx.set_scene(scene)
    fb = torch.zeros(3 * h * w * 3, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device_batch(np.stack([scene.camera, other, scene.camera]), hip.RowSet.whole(w, h), b, spp, fb.data_ptr(), fb.numel() * 8)
    ctx.synchronize()
    assert ctx.batch_info()[0] == 3
    frames = fb.cpu().numpy().reshape(3, h, w, 3)
    assert_is_the_recorded_frame(frames[0], case, want, "batch, frame 0")
    assert_is_the_recorded_frame(frames[2], case, want, "batch, frame 2")
    with np.errstate(all="ignore"):
        between, _ = T.oracle_render(scene.with_camera(other), w, h, b, spp)
    assert np.array_equal(np.isnan(frames[1]), np.isnan(between)), case["name"]
    assert np.array_equal(bits(frames[1])[~np.isnan(between)], bits(between)[~np.isnan(between)]), case["name"]


@gpu
@pytest.mark.parametrize("case", NON_FINITE, ids=[c["name"] for c in NON_FINITE])
def test_the_colour_indices_of_the_non_finite_frames(ctx, case):
    """(int)(c * 255) of a NaN is x86-64's 0x80000000, whose low byte is 0: the device's RGB8 output of the frames that hold NaNs is the
    oracle's quantisation of the recorded frame (of the oracle's own, pinned to the record's hash, where only that is kept)."""
    scene, (want, _) = T.edge_scene(case), oracle_frame(case["name"])
    recorded = T.edge_fb(case)
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_compaction(-1)
    ctx.set_scene(scene)
    got = ctx.render_host_rgb8(scene.camera, hip.RowSet.whole(case["w"], case["h"]), case["b"], case["spp"])
    with np.errstate(all="ignore"):
        assert np.array_equal(got, T.oracle_rgb8(want if recorded is None else recorded)), case["name"]
