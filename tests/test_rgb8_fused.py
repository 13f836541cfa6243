"""The emitter's bytes straight from the ordered mean (trt_render_device_rgb8, trt_render_device_batch_rgb8, trt_render_host_batch_rgb8,
and trt_render_host_rgb8 / trt_render_frame_rgb8 through them): on the production kernel the pass that sums a pixel's samples casts
and stores the bytes itself, a lane per four values and one aligned 32-bit store each, the bytes in front of and behind the aligned
groups one by one.  The expected bytes never come from the library: they are T.oracle_rgb8 -- the CPU checker's (int)(c*255) -- of the
oracle's or the reference's double frame, and the reference's own rgb8_fnv of tests/golden/golden.json."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import support as T
from support import DeviceBytes, anim_cameras, same_bytes
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4


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
        c.set_scratch_fill(False)
        c.set_scene_image(-1)
        c.set_path_patches(-1)
        c.set_compaction(-1)


@functools.lru_cache(maxsize=None)
def scene(kind):
    cam = anim_cameras([0], 160, 48)[0]
    if kind == "demo":
        return S.demo_scene(T.sky("synth"), cam)
    return S.synth_scene({"synth32": 32, "synth64": 64}[kind], T.sky("synth"), cam, seed=11)


@functools.lru_cache(maxsize=None)
def oracle(kind, w, h, index, b, spp):
    """(the oracle's double frame, its bytes by the checker's cast, (path rays, shadow rays)) -- computed once, never written to"""
    px, st = T.oracle_render(scene(kind).with_camera(anim_cameras([index], w, h)[0]), w, h, b, spp)
    rgb = T.oracle_rgb8(px)
    px.flags.writeable = rgb.flags.writeable = False
    return px, rgb, (st.path_rays, st.shadow_rays)


def device_rgb8(ctx, cam, w, h, b, spp, offset=0, rows=None, what=""):
    rows = rows or hip.RowSet.whole(w, h)
    n = hip.lib().trt_rowset_rows(C.byref(rows)) * w * 3
    mem = DeviceBytes(n, offset)
    ctx.render_device_rgb8(cam, rows, b, spp, mem.ptr, n)
    return mem.read(ctx, what).reshape(-1, w, 3)


def batch_rgb8(ctx, cams, w, h, b, spp, offset=0, what=""):
    n = len(cams) * h * w * 3
    mem = DeviceBytes(n, offset)
    ctx.render_batch_rgb8(cams, hip.RowSet.whole(w, h), b, spp, mem.ptr, n)
    return mem.read(ctx, what).reshape(len(cams), h, w, 3)


# ---- 1. the reference's bytes ----

@pytest.mark.parametrize("name", ["demo_160x48_b4", "demo3_160x48_b4"])
def test_device_rgb8_entries_give_the_reference_bytes(ctx, name):
    """the single entry and a batch of one: the reference's rgb8_fnv, and the checker's cast of the reference's double frame"""
    case = next(c for c in T.golden_cases() if c["name"] == name)
    w, h, b, spp = case["width"], case["height"], case["bounce_limit"], case["rays_per_pixel"]
    sc = T.golden_scene(case)
    want = T.oracle_rgb8(T.golden_fb(case)).reshape(h, w, 3)
    assert T.fnv(want) == case["rgb8_fnv"]
    ctx.set_scene(sc)
    single = device_rgb8(ctx, sc.camera, w, h, b, spp, what=name)
    assert T.fnv(single) == case["rgb8_fnv"]
    same_bytes(single, want, name)
    batch = batch_rgb8(ctx, np.array([sc.camera]), w, h, b, spp, what=name + " as a batch of one")
    assert ctx.batch_info() == (1, 1)
    assert T.fnv(batch[0]) == case["rgb8_fnv"]
    same_bytes(batch[0], want, name + " as a batch of one")
    host = ctx.render_host_batch_rgb8(np.array([sc.camera]), hip.RowSet.whole(w, h), b, spp)
    same_bytes(host[0], want, name + " through trt_render_host_batch_rgb8")


# ---- 2. alignment and odd sizes ----

SIZES = [(7, 5, 10), (7, 5, 1), (7, 5, 3), (1, 1, 10), (33, 3, 10), (64, 1, 10)]  # values: 105, 3, 297, 192


@pytest.mark.parametrize("w,h,spp", SIZES, ids=[f"{w}x{h}_spp{s}" for w, h, s in SIZES])
def test_any_alignment_and_any_size(ctx, w, h, spp):
    """every residue of the output address modulo the store's four bytes, frames whose values are no multiple of four and frames
    shorter than a group: the oracle's bytes, and not a byte outside them"""
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[1]
    for offset in range(4):
        same_bytes(device_rgb8(ctx, cam, w, h, 4, spp, offset, what=f"offset {offset}"), want, f"{w}x{h} spp {spp} at offset {offset}")


def test_the_frames_of_a_batch_start_at_any_alignment(ctx):
    """three frames of 105 bytes from offset 1: they start at 1, 106 and 211 bytes behind an aligned address"""
    w, h, indices = 7, 5, [7, 21, 33]
    ctx.set_scene(scene("demo"))
    cams = anim_cameras(indices, w, h)
    for spp in (10, 3):
        got = batch_rgb8(ctx, cams, w, h, 4, spp, offset=1, what=f"batch of 3, spp {spp}")
        assert ctx.batch_info() == (3, 1)
        for k, index in enumerate(indices):
            same_bytes(got[k], oracle("demo", w, h, index, 4, spp)[1], f"frame {k} of the batch, spp {spp}")


ONE = [(67, 13, 3), (5, 1, 1)]  # 2613 values, one more than a multiple of four: a head and a tail at every offset; 15 values: less than a wave


@pytest.mark.parametrize("w,h,spp", ONE, ids=[f"{w}x{h}_spp{s}" for w, h, s in ONE])
def test_a_batch_of_one_is_the_single_frame_entry_at_any_alignment(ctx, w, h, spp):
    """one camera through trt_render_device_batch_rgb8 and through trt_render_device_rgb8 at every residue of the output address: the same
    bytes, the oracle's, and not a byte outside them -- the two entries run ONE kernel, whose grid has exactly a single frame's lanes"""
    assert (w * h * 3) % 4 == 1 or w * h * 3 < 64
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[1]
    for offset in range(4):
        single = device_rgb8(ctx, cam, w, h, 4, spp, offset, what=f"single, offset {offset}")
        batch = batch_rgb8(ctx, np.array([cam]), w, h, 4, spp, offset, what=f"batch of one, offset {offset}")
        assert ctx.batch_info() == (1, 1)
        same_bytes(batch[0], single, f"{w}x{h} spp {spp}: a batch of one against the single entry at offset {offset}")
        same_bytes(single, want, f"{w}x{h} spp {spp} at offset {offset}")


# ---- 3. every output kind on one context ----

def test_every_output_kind_interleaved_on_one_context():
    """doubles and bytes, single frames and batches, host and device entries in turn: a queue one kind leaves unready for the next, a
    scratch sized for the other kind or a history entry left open would show in a frame or in the count of kernel times"""
    w, h, b, spp = 160, 48, 4, 3
    rows = hip.RowSet.whole(w, h)
    indices = [0, 19, 59]
    cams = anim_cameras(indices, w, h)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    px = [oracle("synth64", w, h, i, b, spp)[0] for i in indices]
    rgb = [oracle("synth64", w, h, i, b, spp)[1] for i in indices]
    with hip.Context(0) as c:
        c.set_scene(scene("synth64"))
        calls = 0
        for turn in range(2):
            assert np.array_equal(bits(c.render_host(cams[0], rows, b, spp)), bits(px[0])), turn
            same_bytes(c.render_host_rgb8(cams[1], rows, b, spp), rgb[1], f"render_host_rgb8, turn {turn}")
            same_bytes(device_rgb8(c, cams[2], w, h, b, spp, offset=turn + 1), rgb[2], f"render_device_rgb8, turn {turn}")
            got = batch_rgb8(c, cams, w, h, b, spp, offset=3 - turn)
            assert c.batch_info() == (3, 1)
            for k in range(3):
                same_bytes(got[k], rgb[k], f"render_batch_rgb8 frame {k}, turn {turn}")
            frames = c.render_host_batch(cams, rows, b, spp)
            for k in range(3):
                assert np.array_equal(bits(frames[k]), bits(px[k])), (turn, k)
            same_bytes(c.render_host_rgb8(cams[0], rows, b, spp), rgb[0], f"render_host_rgb8 after a batch, turn {turn}")
            got = c.render_host_batch_rgb8(cams[::-1].copy(), rows, b, spp)
            for k in range(3):
                same_bytes(got[k], rgb[2 - k], f"render_host_batch_rgb8 frame {k}, turn {turn}")
            calls += 7
            assert c.launch_count() == calls
        times = c.kernel_times()
        assert len(times) == calls and all(t > 0 for t in times)
        render_ms, reduce_ms = c.render_kernel_times()
        assert len(render_ms) == calls and all(t > 0 for t in render_ms) and all(t > 0 for t in reduce_ms)


# ---- 4. the instantiations ----

def _decoupled(c):
    c.set_compaction(1)
    return "synth64", lambda: c.render_variant()["decoupled"]


def _patches(c):
    c.set_path_patches(2)
    return "synth32", lambda: c.path_patches()[0] == 2 and c.render_variant()["workgroup_threads"] in (256, 1024)


def _image(c):
    c.set_scene_image(1)
    return "synth64", lambda: c.render_image()["in_device_memory"]


def _counting(c):
    c.enable_counters(True)
    return "synth64", lambda: True


def _reference(c):
    c.set_kernel(hip.Context.REFERENCE_ORDER)
    return "synth64", lambda: c.render_variant()["workgroup_threads"] == 256


@pytest.mark.parametrize("setup", [_decoupled, _patches, _image, _counting, _reference], ids=lambda f: f.__name__.strip("_"))
def test_the_byte_path_through_every_instantiation(ctx, setup):
    w, h, b, spp, index = 96, 32, 4, 3, 19
    kind, ran = setup(ctx)
    ctx.set_scene(scene(kind))
    cam = anim_cameras([index], w, h)[0]
    _, want, counts = oracle(kind, w, h, index, b, spp)
    same_bytes(device_rgb8(ctx, cam, w, h, b, spp, offset=1, what=setup.__name__), want, setup.__name__ + ", device entry")
    assert ran(), setup.__name__
    if setup is _counting:
        assert ctx.read_counters() == counts
    same_bytes(ctx.render_host_rgb8(cam, hip.RowSet.whole(w, h), b, spp), want, setup.__name__ + ", host entry")
    rows = hip.RowSet.shard(w, h, 1, 3, 4)
    owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(hip.lib().trt_rowset_rows(C.byref(rows)))]
    same_bytes(device_rgb8(ctx, cam, w, h, b, spp, offset=2, rows=rows), want[owned], setup.__name__ + ", a shard")


def test_a_batch_served_one_launch_per_camera_writes_each_frame_at_its_offset(ctx):
    """the device image has no BATCH form: two launches, the second frame 96 * 32 * 3 bytes behind the first"""
    w, h, b, spp, indices = 96, 32, 4, 3, [19, 41]
    ctx.set_scene_image(1)
    ctx.set_scene(scene("synth64"))
    got = batch_rgb8(ctx, anim_cameras(indices, w, h), w, h, b, spp, offset=3)
    assert ctx.batch_info() == (2, 2) and ctx.render_image()["in_device_memory"]
    for k, index in enumerate(indices):
        same_bytes(got[k], oracle("synth64", w, h, index, b, spp)[1], f"frame {k}")
    ctx.set_kernel(hip.Context.REFERENCE_ORDER)  # likewise the reference-order kernel, through the context's framebuffer
    got = ctx.render_host_batch_rgb8(anim_cameras(indices, w, h), hip.RowSet.whole(w, h), b, spp)
    assert ctx.batch_info() == (2, 2)
    for k, index in enumerate(indices):
        same_bytes(got[k], oracle("synth64", w, h, index, b, spp)[1], f"reference-order kernel, frame {k}")


# ---- 5. the cast's corners ----

def test_a_filled_scratch_and_a_filled_output_leave_the_oracles_bytes(ctx):
    """trt_set_scratch_fill: the launch's samples and its output bytes are 0xFF before the launch -- a NaN in every double, which the
    cast turns into 0 -- so a sample the render kernel drops or a byte the fused pass skips shows; exactly the frame's bytes are filled"""
    ctx.set_scratch_fill(True)
    ctx.set_scene(scene("demo"))
    for w, h, spp in ((67, 13, 10), (7, 5, 3)):
        cam = anim_cameras([7], w, h)[0]
        want = oracle("demo", w, h, 7, 4, spp)[1]
        assert (want != 0xFF).any() and (want != 0).any()
        for offset in (0, 3):
            same_bytes(device_rgb8(ctx, cam, w, h, 4, spp, offset, what="filled"), want, f"filled, {w}x{h} at offset {offset}")
        same_bytes(ctx.render_host_rgb8(cam, hip.RowSet.whole(w, h), 4, spp), want, f"filled, {w}x{h}, host entry")
    w, h, indices = 7, 5, [7, 21, 33]
    got = batch_rgb8(ctx, anim_cameras(indices, w, h), w, h, 4, 3, offset=2, what="filled batch")
    for k, index in enumerate(indices):
        same_bytes(got[k], oracle("demo", w, h, index, 4, 3)[1], f"filled batch, frame {k}")
    ctx.set_kernel(hip.Context.REFERENCE_ORDER)
    same_bytes(device_rgb8(ctx, anim_cameras([7], 7, 5)[0], 7, 5, 4, 3, offset=1, what="filled, reference-order"), oracle("demo", 7, 5, 7, 4, 3)[1],
               "filled, reference-order kernel")


# ---- 6. errors ----

def test_refusals_enqueue_nothing_and_leave_the_context_rendering(ctx):
    import torch
    lib = hip.lib()
    w, h, b, spp = 33, 3, 4, 3
    rows, bad_rows = hip.RowSet.whole(w, h), hip.RowSet(0, h, h, 0, 1)
    cams = anim_cameras([7, 21], w, h)
    cam = hip.camera_struct(cams[0])
    n = w * h * 3
    mem = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    host = np.full(2 * n, 0xA5, dtype=np.uint8)
    torch.cuda.synchronize()
    p, hp, cp, r = C.c_void_p(mem.data_ptr()), C.c_void_p(host.ctypes.data), C.c_void_p(cams.ctypes.data), C.byref(rows)
    with hip.Context(0) as empty:
        assert lib.trt_render_device_rgb8(empty._h, C.byref(cam), r, b, spp, p, n) == NO_SCENE
        assert lib.trt_render_device_batch_rgb8(empty._h, cp, 2, r, b, spp, p, 2 * n) == NO_SCENE
        assert lib.trt_render_host_batch_rgb8(empty._h, cp, 2, r, b, spp, hp) == NO_SCENE
        assert lib.trt_render_host_rgb8(empty._h, C.byref(cam), r, b, spp, hp) == NO_SCENE
    ctx.set_scene(scene("demo"))
    h_ = ctx._h
    single = lambda c=h_, camera=C.byref(cam), rs=r, bl=b, out=p, cap=n: lib.trt_render_device_rgb8(c, camera, rs, bl, spp, out, cap)
    batch = lambda c=h_, cameras=cp, k=2, rs=r, bl=b, out=p, cap=2 * n: lib.trt_render_device_batch_rgb8(c, cameras, k, rs, bl, spp, out, cap)
    hbatch = lambda c=h_, cameras=cp, k=2, rs=r, bl=b, out=hp: lib.trt_render_host_batch_rgb8(c, cameras, k, rs, bl, spp, out)
    for entry in (single, batch, hbatch):
        assert entry(c=None) == ARGUMENT and entry(out=None) == ARGUMENT
        assert entry(rs=C.byref(bad_rows)) == ARGUMENT and entry(rs=None) == ARGUMENT
        assert entry(bl=0) == ARGUMENT
    assert single(camera=None) == ARGUMENT
    other = cams.copy()
    other[1, 13] *= 2
    for entry in (batch, hbatch):
        assert entry(cameras=None) == ARGUMENT
        assert entry(k=0) == ARGUMENT and entry(k=9) == ARGUMENT
        assert entry(cameras=C.c_void_p(other.ctypes.data)) == ARGUMENT
    assert single(cap=n - 1) == CAPACITY and batch(cap=2 * n - 1) == CAPACITY
    assert single(cap=n) == 0 and batch(cap=2 * n) == 0  # to the byte
    ctx.synchronize()
    assert (host == 0xA5).all(), "a refused host entry wrote to the caller's buffer"
    got = mem.cpu().numpy().reshape(2, h, w, 3)
    for k, index in enumerate((7, 21)):
        same_bytes(got[k], oracle("demo", w, h, index, 4, spp)[1], f"the good call after the refusals, frame {k}")
    same_bytes(ctx.render_host_batch_rgb8(cams, rows, b, spp)[1], oracle("demo", w, h, 21, 4, spp)[1], "the host batch after the refusals")
