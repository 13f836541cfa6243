"""The camera's value domain against the reference's OWN frames (tests/golden/camera_edges.npz, golden_camera_edges.json, recorded by
tests/golden/make_golden_cameras.py from the compiled reference): screen distances, screen sizes, bases and eyes outside the domain of
bench_camera(), which is all the rest of the suite renders with -- an orthonormal basis, screen_distance 1, screen_height 5,
screen_width 5 W / H.

The primary ray of TRT.c:981-1011 is formed in three places (primary_direction for the reference-order kernel; the production rounds
from host-made axes, a host-made jitter table and basis z * -screen_distance staged once per workgroup; the batch image from cameras
passed by value), behind three host caches keyed by == on doubles.  A product that is right only at screen_distance 1, a basis taken
for orthonormal, a table left stale when one screen field changes or a sign lost at -0.0 would pass every other test.

A camera is `defined` where every primary direction is finite and not of zero length: the reference's two builds then agree bit for
bit and the record holds the frame.  On the others the reference indexes outside its tables and dies; they are recorded by name, and
judged by the oracle under the library's own definitions (the last test of this file)."""
import ctypes as C
import functools

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import hip
from support import KERNEL_IDS, KERNELS, bits, render

gpu = pytest.mark.gpu
CASES = T.camera_cases()
IDS = [c["name"] for c in CASES]
BUILT = T.camera_scenes()
DEFINED = [name for name, *_, defined in BUILT if defined]
UNDEFINED = [name for name, *_, defined in BUILT if not defined]
MAX_NAN_SHARE = 0.10
FIRST = T.VALUE_SHOTS[0]
ARGUMENT = -2

# cameras that legitimately give ONE frame, bit for bit, at every shot (and so cannot tell each other apart):
#  - a screen_distance of +0, -0 and 1e-300: basis z * -screen_distance is +-0 or below half an ulp of every other term;
#  - a mirrored screen and a mirrored x axis: (-x) sx and x (-sx) are the same products, the jitter's sign included;
#  - no screen height and no y axis: y * 0 and 0 * sy are the same zeros;
#  - a screen of denormal size, a zero basis and a basis of 1e-200: the screen point vanishes against the eye, every ray is -eye;
#  - an eye at the origin and an eye a denormal from it: the eye vanishes against the screen point and against every hit point.
SAME_FRAME = [{"screen_distance 0.0", "screen_distance -0.0", "screen_distance 1e-300"},
              {"screen_width negated", "basis left-handed"},
              {"screen_height 0", "basis y = 0"},
              {"screen_width 5e-324, screen_height 1e-310", "basis all zero", "basis x1e-200"},
              {"eye at the origin", "eye a denormal from the origin"}]


def case_of(camera, shot=FIRST):
    return next(c for c in CASES if c["camera"] == camera and (c["b"], c["spp"]) == tuple(shot))


@functools.lru_cache(maxsize=None)
def oracle_of(camera_bytes, w, h, b, spp):
    """the oracle's frame of the family's scene under a camera: rendered once, shared by the tests, never written to"""
    scene = BUILT[0][1].with_camera(np.frombuffer(camera_bytes, dtype=np.float64))
    with np.errstate(all="ignore"):
        px, st = T.oracle_render(scene, w, h, b, spp)
    px.flags.writeable = False
    return px, st


def oracle_frame(case):
    return oracle_of(T.camera_case_scene(case).camera.tobytes(), case["w"], case["h"], case["b"], case["spp"])


def is_recorded(got, case, who):
    T.assert_is_the_recorded_frame(got, case, T.camera_fb(case), oracle_frame(case)[0], who)


# ---- CPU: the fixture is what it claims, and the oracle equals it ----

def test_the_record_is_what_it_claims():
    """Counts and hashes are those of the stored frames; no defined frame holds a NaN (the cap is the project's tenth, the reference's
    frames had none); every camera the builder calls defined is recorded at both shots, every other one by name in `undefined`, with
    what the reference did; none was dropped."""
    assert "No camera was dropped" in T.camera_meta()["note"]
    assert [(c["camera"], c["b"], c["spp"]) for c in CASES] == [(n, b, s) for n in DEFINED for b, s in T.VALUE_SHOTS]
    assert [u["name"] for u in T.camera_meta()["undefined"]] == UNDEFINED
    assert all("signal" in u["what"] or "differ" in u["what"] for u in T.camera_meta()["undefined"])
    assert len(DEFINED) >= 29 and len(UNDEFINED) >= 14
    for c in CASES:
        assert c["nan"] <= MAX_NAN_SHARE * c["w"] * c["h"] * 3 and c["nan"] == 0, c["name"]
        assert (c["w"], c["h"]) in ((48, 27), (96, 27))
        fb = T.camera_fb(c)
        if fb is not None:
            assert (c["b"], c["spp"]) == FIRST
            assert (int(np.isnan(fb).sum()), int(np.isinf(fb).sum())) == (c["nan"], c["inf"]) and T.fnv(T.canonical_nans(fb)) == c["fb_fnv"], c["name"]
            assert int(np.unique(bits(fb)).size) == c["distinct"], c["name"]
    for name in (T.CAMERA_BASE, T.CAMERA_WIDE) + T.CAMERA_TRIO:  # what the chain, batch and shard tests render first
        assert T.camera_fb(case_of(name)) is not None, name


def test_the_builders_still_make_the_recorded_cameras():
    """Bit for bit, signed zeros and NaNs included, for the defined cameras and for those the reference dies on; and one scene under
    all of them."""
    archive = T._camera_edges()
    for name, scene, w, h, defined in BUILT:
        assert np.array_equal(bits(archive["cam/" + name]), bits(scene.camera)), name
        assert np.array_equal(bits(T.pack_scene(scene))[:-15], bits(archive["scene"])[:-15]), name
    for c in CASES:
        name, scene, w, h, _ = next(b for b in BUILT if b[0] == c["camera"])
        assert (w, h) == (c["w"], c["h"])
        assert np.array_equal(bits(T.pack_scene(T.camera_case_scene(c))), bits(T.pack_scene(scene))), c["name"]
    assert np.signbit(archive["cam/screen_distance -0.0"][12]) and not np.signbit(archive["cam/screen_distance 0.0"][12])
    trio = [archive["cam/" + n] for n in T.CAMERA_TRIO]
    assert all(np.array_equal(bits(t[12:15]), bits(trio[0][12:15])) for t in trio) and trio[0][12] == 0.05 and trio[0][13] < 0 and trio[0][14] == 3.0
    assert len({t[:12].tobytes() for t in trio}) == 3 and len({t[9:12].tobytes() for t in trio}) == 3


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_equals_the_reference_frame(case):
    px, st = oracle_frame(case)
    is_recorded(px, case, "oracle")
    assert st.samples == case["w"] * case["h"] * case["spp"]


def _unit_or_itself(v):
    n = np.sqrt(v @ v)
    return v / n if n > 0 and np.isfinite(n) else v


def _orthogonalised(basis):
    x, y, z = basis.reshape(3, 3)
    ux = _unit_or_itself(x)
    y = y - (y @ ux) * ux
    uy = _unit_or_itself(y)
    z = z - (z @ ux) * ux - (z @ uy) * uy
    return np.concatenate([x, y, z])


# what a kernel could take a camera for and still pass every test that renders with bench_camera(): name -> the camera it would render
MISTAKES = {
    "screen_distance taken as 1": lambda cam, w, h: np.concatenate([cam[:12], [1.0], cam[13:]]),
    "screen_height taken as 5": lambda cam, w, h: np.concatenate([cam[:14], [5.0]]),
    "screen_width taken as 5 W / H": lambda cam, w, h: np.concatenate([cam[:13], [5 * float(w) / float(h)], cam[14:]]),
    "basis vectors normalised": lambda cam, w, h: np.concatenate([np.concatenate([_unit_or_itself(v) for v in cam[:9].reshape(3, 3)]), cam[9:]]),
    "basis orthogonalised": lambda cam, w, h: np.concatenate([_orthogonalised(cam[:9]), cam[9:]]),
    "basis transposed": lambda cam, w, h: np.concatenate([cam[:9].reshape(3, 3).T.ravel(), cam[9:]]),
}


def test_the_cases_bite(capsys):
    """Every mistake of MISTAKES, substituted into the oracle, changes the frame of at least one recorded case (which ones is printed);
    every camera's frame differs from the base camera's; and the cameras that share a frame are exactly the groups of SAME_FRAME."""
    firsts = [case_of(name) for name in DEFINED]
    caught = {}
    for mistake, wrong in MISTAKES.items():
        caught[mistake] = []
        for c in firsts:
            cam = T.camera_case_scene(c).camera
            taken = np.ascontiguousarray(wrong(cam, c["w"], c["h"]))
            if np.array_equal(bits(taken), bits(cam)):
                continue
            px, _ = oracle_of(taken.tobytes(), c["w"], c["h"], c["b"], c["spp"])
            if T.fnv(T.canonical_nans(px)) != c["fb_fnv"]:
                caught[mistake].append(c["camera"])
    with capsys.disabled():
        for mistake, names in caught.items():
            print(f"\n{mistake}: caught by {len(names)} cases: {'; '.join(names)}", end="")
        print()
    for mistake, names in caught.items():
        assert names, mistake
    for shot in T.VALUE_SHOTS:
        by_hash = {}
        for name in DEFINED:
            by_hash.setdefault(case_of(name, shot)["fb_fnv"], set()).add(name)
        assert by_hash[case_of(T.CAMERA_BASE, shot)["fb_fnv"]] == {T.CAMERA_BASE}, shot
        shared = sorted((g for g in by_hash.values() if len(g) > 1), key=sorted)
        assert shared == sorted(SAME_FRAME, key=sorted), (shot, shared)


# ---- GPU ----

@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.set_path_grids_min_spheres(0)
    c.set_scratch_fill(True)  # a unit a launch drops reads as a NaN, and no defined frame has one
    yield c
    c.close()


ALL_KERNELS = list(zip(KERNELS, KERNEL_IDS)) + [(hip.Context.PRODUCTION, "production_rounds, device image")]


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_kernel_equals_the_reference_frame(ctx, case):
    """The production kernel as it ships, with the decoupling forced and the reference-order kernel, then the production kernel
    reading the scene from device memory; the trace counts are the oracle's."""
    scene, (want, st) = T.camera_case_scene(case), oracle_frame(case)
    w, h, b, spp = case["w"], case["h"], case["b"], case["spp"]
    ctx.enable_counters(True)
    try:
        for kernel, who in ALL_KERNELS:
            in_device_memory = who.endswith("device image")
            ctx.set_scene_image(1 if in_device_memory else -1)
            got = render(ctx, scene, w, h, b, spp, kernel)
            if in_device_memory:
                assert ctx.render_image()["in_device_memory"], who
            is_recorded(got, case, who)
            assert ctx.read_counters() == (st.path_rays, st.shadow_rays), (case["name"], who)
    finally:
        ctx.enable_counters(False)
        ctx.set_scene_image(-1)


# neighbours differ in exactly one thing: screen_distance, its sign at zero, screen_width, screen_height, the basis under one eye, the
# eye, and (base <-> the 96-column case) the axes under one pixel width, that is, one jitter table
CHAIN = [T.CAMERA_BASE, "screen_distance 0.05", "screen_distance 0.0", "screen_distance -0.0", "screen_distance 40.0", "screen_distance -1.0", T.CAMERA_BASE,
         "screen_width negated", "screen_width 0", T.CAMERA_BASE, "screen_height -5", "screen_height 0", T.CAMERA_BASE,
         "basis x3", "basis sheared", "basis rolled 37 degrees", "basis singular", T.CAMERA_BASE,
         "eye at the origin", "eye a denormal from the origin", T.CAMERA_BASE, T.CAMERA_WIDE, T.CAMERA_BASE]


def test_neighbours_of_the_chain_differ_in_one_thing():
    fields = {"basis": slice(0, 9), "eye": slice(9, 12), "screen_distance": slice(12, 13), "screen_width": slice(13, 14), "screen_height": slice(14, 15)}
    seen = set()
    for a, b in zip(CHAIN, CHAIN[1:]):
        ca, cb = (T.camera_case_scene(case_of(n)).camera for n in (a, b))
        changed = [k for k, s in fields.items() if not np.array_equal(bits(ca[s]), bits(cb[s]))]
        assert len(changed) == 1, (a, b, changed)
        seen.add("columns" if T.CAMERA_WIDE in (a, b) else "sign of zero" if ca[12] == cb[12] and changed == ["screen_distance"] else changed[0])
    assert seen == set(fields) | {"columns", "sign of zero"}
    wide, base = case_of(T.CAMERA_WIDE), case_of(T.CAMERA_BASE)
    cw, cb = T.camera_case_scene(wide).camera, T.camera_case_scene(base).camera
    assert cw[13] / wide["w"] == cb[13] / base["w"] and cw[14] / wide["h"] == cb[14] / base["h"]  # prepare_jitter's key


@gpu
@pytest.mark.parametrize("kernel", [hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER], ids=["production_rounds", "reference_order"])
def test_the_host_tables_follow_the_camera_on_one_context(kernel):
    """The chain forward, then backward, on a context of its own (its jitter, axes and eye slots have seen nothing else): every frame
    is its record, and so is a frame of the first camera at the end."""
    with hip.Context(0) as ctx:
        ctx.set_path_grids_min_spheres(0)
        ctx.set_scratch_fill(True)
        ctx.set_kernel(kernel)
        ctx.set_scene(BUILT[0][1])
        for step, name in enumerate(CHAIN + CHAIN[::-1][1:] + [CHAIN[0]]):
            case = case_of(name)
            got = ctx.render_host(T.camera_case_scene(case).camera, hip.RowSet.whole(case["w"], case["h"]), case["b"], case["spp"])
            is_recorded(got, case, f"step {step}")


def configure_variant(ctx, variant):
    from test_work_units import SETTINGS
    kernel, compaction, m, image, _, _ = SETTINGS[variant]
    ctx.set_kernel(kernel)
    ctx.set_compaction(compaction)
    ctx.set_scene_image(image)
    ctx.set_path_patches(m)


@gpu
@pytest.mark.parametrize("variant", ["plain", "patches", "decoupled"])  # the batch forms of test_work_units.py
def test_a_batch_of_three_bases_on_one_odd_screen(variant):
    """trt_render_device_batch with the trio -- rolled, sheared and left-handed x3 bases with an eye each, on a screen at distance 0.05
    that is mirrored and 3 high -- in ONE launch of the variant asked for: three records."""
    import torch
    from test_work_units import expected, ran
    cases = [case_of(n) for n in T.CAMERA_TRIO]
    w, h, b, spp = (cases[0][k] for k in ("w", "h", "b", "spp"))
    cams = np.stack([T.camera_case_scene(c).camera for c in cases])
    with hip.Context(0) as ctx:
        ctx.set_path_grids_min_spheres(0)
        ctx.set_scratch_fill(True)
        configure_variant(ctx, variant)
        ctx.set_scene(BUILT[0][1])
        for order in ([0, 1, 2], [2, 0, 1]):
            fb = torch.zeros(3 * h * w * 3, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.render_device_batch(cams[order], hip.RowSet.whole(w, h), b, spp, fb.data_ptr(), fb.numel() * 8)
            ctx.synchronize()
            assert ctx.batch_info() == (3, 1), (variant, ctx.batch_info())
            assert ran(ctx) == expected(variant), (variant, ran(ctx))
            frames = fb.cpu().numpy().reshape(3, h, w, 3)
            for k, i in enumerate(order):
                is_recorded(frames[k], cases[i], f"{variant}, frame {k} of {order}")


@gpu
def test_a_batch_refuses_another_screen_and_serves_both_zeros(ctx):
    """A batch whose camera 1 differs from camera 0 in screen_distance alone, in screen_width alone or in screen_height alone is refused
    with TRT_ERR_ARGUMENT before anything is enqueued: the framebuffer keeps its zeros, the launch count stands, the context renders
    on.  +0.0 and -0.0 compare equal: a batch of both is served, and each frame is the record of its own camera (and the oracle's)."""
    import torch
    base = case_of(T.CAMERA_BASE)
    w, h, b, spp = (base[k] for k in ("w", "h", "b", "spp"))
    rows = hip.RowSet.whole(w, h)
    cam = T.camera_case_scene(base).camera
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_compaction(-1)
    ctx.set_scene(BUILT[0][1])
    is_recorded(ctx.render_host(cam, rows, b, spp), base, "before the refusals")
    for other in ("screen_distance 0.05", "screen_width negated", "screen_height -5"):
        second = T.camera_case_scene(case_of(other)).camera
        assert int((bits(second) != bits(cam)).sum()) == 1, other
        for cams in (np.stack([cam, second]), np.stack([second, cam]), np.stack([cam, cam, second])):
            fb = torch.zeros(len(cams) * h * w * 3, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            launches = ctx.launch_count()
            with pytest.raises(hip.TrtError) as e:
                ctx.render_device_batch(cams, rows, b, spp, fb.data_ptr(), fb.numel() * 8)
            assert e.value.code == ARGUMENT, (other, e.value)
            assert "screen_width / screen_height / screen_distance" in str(e.value)
            ctx.synchronize()
            assert ctx.launch_count() == launches, other
            assert not fb.cpu().numpy().any(), other
    is_recorded(ctx.render_host(cam, rows, b, spp), base, "after the refusals")
    zeros = [case_of("screen_distance 0.0"), case_of("screen_distance -0.0")]
    cams = np.stack([T.camera_case_scene(c).camera for c in zeros] * 2)[:3]  # +0, -0, +0
    assert [bool(np.signbit(c[12])) for c in cams] == [False, True, False]
    got = ctx.render_host_batch(cams, rows, b, spp)
    assert ctx.batch_info() == (3, 1)
    for k in range(3):
        is_recorded(got[k], zeros[k % 2], f"frame {k} of +0, -0, +0")
        assert np.array_equal(bits(got[k]), bits(oracle_frame(zeros[k % 2])[0])), k


@gpu
@pytest.mark.parametrize("kernel", [hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER], ids=["production_rounds", "reference_order"])
def test_shards_index_the_rows_of_another_screen_height(ctx, kernel):
    """The trio's rolled camera (screen_height 3, a mirrored screen) on interleaved tiles of 5 rows over 3 ranks: row_y is indexed by
    the FRAME row (frame_row_of_magic); the shards reassemble to the record."""
    case = case_of(T.CAMERA_TRIO[0])
    scene, w, h = T.camera_case_scene(case), case["w"], case["h"]
    out = np.full((h, w, 3), np.nan)
    for rank in range(3):
        rs = hip.RowSet.shard(w, h, rank, 3, 5)
        part = render(ctx, scene, w, h, case["b"], case["spp"], kernel, rows=rs)
        for i in range(part.shape[0]):
            out[hip.lib().trt_rowset_frame_row(C.byref(rs), i)] = part[i]
    is_recorded(out, case, "reassembled")


# ---- cameras the reference does not define: the library's definitions, stated by the oracle, judge the kernels ----
# A primary direction that is not finite or of zero length ends on the sky (no sphere and no plane test passes with it), where
# get_skybox_color (TRT.c:700-789) indexes outside its tables.  The library defines (csrc/trt_device.hpp, sky_texel):
#  - a direction with a NaN component wins no face (every dot product with an axis is NaN): face 0, not face -1;
#  - a texel index past the face's last texel is the last texel, one below zero is texel 0.  A NaN or zero direction has NaN face
#    coordinates, whose (int) conversion is x86-64's 0x80000000: below zero, so texel 0.
SKY_CORNERS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1), (-1, 1, 1), (-1, 1, -1), (-1, -1, 1), (-1, -1, -1)]
DEGENERATE = [(np.nan, 0.5, 0.2), (0.5, np.nan, 0.2), (0.5, 0.2, np.nan), (np.nan, np.nan, np.nan), (np.nan, 0.0, 0.0), (0.0, -0.0, np.nan),
              (0.0, 0.0, 0.0), (-0.0, 0.0, -0.0), (1e-320, 0.0, 0.0)]
DEGENERATE_UNIT = DEGENERATE[:-1]  # the last is a direction only before unit() (it is left alone, and 1 / 1e-320 is infinite)


def test_the_oracle_states_the_library_s_definitions():
    """trt_oracle_skybox_lookup: face 0 and an index below zero for every degenerate direction, an index past the face for some
    corner of the cube; and through trt_oracle_trace_ray the texels those stand for: texel 0 of face +X, the face's last texel."""
    scene = BUILT[0][1]
    sc, lib, dim = scene.as_scene(), T.oracle(), scene.sky_dim
    looked = {}
    for d in SKY_CORNERS + DEGENERATE:
        v, face, idx = np.array(d, dtype=np.float64), C.c_int(-7), C.c_long(-7)
        inside = lib.trt_oracle_skybox_lookup(C.byref(sc), T.L.Vector.from_buffer(v), C.byref(face), C.byref(idx))
        looked[d] = (inside, face.value, idx.value)
    for d in DEGENERATE:
        assert looked[d][:2] == (0, 0) and looked[d][2] < 0, (d, looked[d])
    past = [d for d in SKY_CORNERS if looked[d][0] == 0]
    assert past and all(looked[d][2] >= dim * dim for d in past), looked
    up = [d for d in past if d[1] > 0] + DEGENERATE  # from 100 above the scene these rays meet nothing
    rays = np.array([[0.0, 100.0, 0.0, *d] for d in up])
    with np.errstate(all="ignore"):
        out = T.oracle_probe(scene, rays)
    assert (out["obj"] == T.L.NONE).all()
    for d, colour in zip(up, out["material"][:, :3]):
        face = looked[d][1]
        texel = scene.sky[face].reshape(-1, 3)[-1 if d in past else 0]
        assert np.array_equal(colour, texel / 255.0), (d, colour, texel)


def undefined_frames():
    """[(name, scene, w, h, b, spp, the oracle's frame, its counts)]: rendered once, after the definitions above are shown to hold"""
    out = []
    for name, scene, w, h, defined in BUILT:
        if not defined:
            for b, spp in T.VALUE_SHOTS:
                want, st = oracle_of(scene.camera.tobytes(), w, h, b, spp)
                out.append((name, scene, w, h, b, spp, want, (st.path_rays, st.shadow_rays)))
    return out


def test_the_undefined_cameras_end_on_texel_0_of_face_0():
    """What the definitions make of them, in the oracle: no NaN in any frame; where every primary direction is degenerate the frame
    is one colour, texel 0 of face +X; the two cameras with ONE zero-length ray (48x28, the first ray of a pixel) are ordinary
    frames but for that ray."""
    texel = BUILT[0][1].sky[0, 0, 0] / 255.0
    for name, scene, w, h, b, spp, want, (path, _) in undefined_frames():
        assert np.isfinite(want).all(), name
        if (w, h) == (48, 28):
            assert np.unique(bits(want)).size > 100, name
        else:
            mean = (texel * spp) * (1.0 / spp) if spp == 1 else ((texel + texel) + texel) * (1.0 / spp)  # TRT.c:1065, in its order
            assert np.array_equal(want, np.broadcast_to(mean, want.shape)) and path == w * h * spp, (name, spp)


@gpu
def test_the_sky_look_up_of_a_degenerate_direction(ctx):
    """sky_index_estimate must not vouch for a direction with a NaN component (v_min_f32 drops a NaN operand: a NaN coordinate beside
    a good one used to pass as `sure`), and sky_index_unit gives texel 0 of face 0 for it, as sky_texel does; a zero direction
    likewise.  Run before the cameras below, whose frames rest on it."""
    dirs = np.array(DEGENERATE_UNIT, dtype=np.float64)
    for dim in (1, 64, 2048):
        exact, est, amb = ctx.selftest_sky(dirs, dim)
        assert amb.all(), (dim, amb.tolist())
        assert not exact.any(), (dim, exact.tolist())


@gpu
def test_cameras_the_reference_does_not_define(ctx):
    """Every kernel and the device-image form on the cameras the reference dies on, against the oracle: NaNs in the same places
    (there are none), the bits of every other value, the trace counts.

    Why every index stays in range with a direction d that has a NaN component or is (0, 0, 0) (an infinite component does not
    outlive unit(): inf / inf is NaN, x / inf is 0), read from the code before the first run:
     - unit(): arithmetic only; a NaN or infinite length fails `ok`, the wave takes the compiler's divisions.
     - primary ray: col_x, row_y and the jitter are indexed by column, frame row and sample number, never by a value.
     - path_cell / path_cell_patches: the table is read only under `member`, which needs |d.d - 1| <= 2^-40 -- false for NaN and
       for zero, and every other compare with a NaN eye is false too; the lane falls back, so its whole wave sweeps.  The cell
       number is formed anyway: face from v_cubeid (0..5 for any input, NaN compares are false), coordinates through
       fmin(fmax(x, 0), g - 1), which turns NaN into 0.  The eye's families with a NaN or infinite apex are built by a kernel
       indexed by cell number; their cones say `everywhere` (trt_rayfamily_cone: "also for D = 0 and NaN") and the pool hands out
       no word past the slot's limit (pack_cell).
     - the filter sweep: indexed by sphere number up to cull.padded, candidates are tested only below n; with a = d.d = 0 the
       discriminant is b * b = 0 and b < 0 fails, with NaN every compare fails; the plane test needs |d.n| > 1e-5.  So the ray
       ends on the sky, no material or light table is read for it (the checker parity of a NaN point is d2i's 0x80000000 & 1 = 0).
     - sky_texel_wave: the estimate's index is used only for a lane that is `sure`: face 0..5 and both coordinates inside
       (e, dim - e); a NaN coordinate is never sure (the test above).  Every other lane takes sky_index_unit: face 0..5 and
       an index clamped to [0, dim * dim - 1].  sky_texel (reference-order kernel): face -1 becomes 0, the same clamp."""
    ctx.enable_counters(True)
    try:
        for name, scene, w, h, b, spp, want, counts in undefined_frames():
            for kernel, who in ALL_KERNELS:
                ctx.set_scene_image(1 if who.endswith("device image") else -1)
                got = render(ctx, scene, w, h, b, spp, kernel)
                what = (name, b, spp, who)
                assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaNs in other places", int(np.isnan(got).sum()))
                assert np.array_equal(bits(got), bits(want)), (what, int((bits(got) != bits(want)).sum()), got[0, 0].tolist(), want[0, 0].tolist())
                assert ctx.read_counters() == counts, what
    finally:
        ctx.enable_counters(False)
        ctx.set_scene_image(-1)
