"""The frame as a kitty graphics-protocol image written on the device (trt_render_device_kitty, trt_render_device_batch_kitty,
trt_render_host_kitty, trt_render_host_batch_kitty, trt_render_frame_kitty, trt_kitty_from_rgb8_device): behind the production kernel the
pass that sums a pixel's samples casts it to the emitter's bytes, forms its four base64 characters and stores the text itself, a wave per
64 aligned 32-bit words (csrc/trt_kitty.h, trt_kitty.hpp).  The expected bytes never come from the library's device route: they are the
sequential host emitter's (host.emitter_kitty_rgb8, which tests/test_kitty_layout.py holds against a formatter around the standard
library's base64, a literal and a structural reader) of T.oracle_rgb8 -- the CPU checker's (int)(c*255) -- of the oracle's double frame,
and the structural reader (tests/kitty_support.py) reads every device text back to those bytes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import kitty_support as K
import support as T
from support import STORE, DeviceBytes, anim_cameras, owned_rows
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4
# (width, rows, bounce limit, rays per pixel): P on the wave's and the chunk's edges -- 1, 63, 64, 65, 1023, 1024, 1025, 2049 -- and 160 x 48
SHAPES = [(1, 1, 2, 3), (21, 3, 2, 3), (8, 8, 2, 3), (13, 5, 2, 3), (341, 3, 2, 3), (32, 32, 2, 3), (41, 25, 2, 3), (683, 3, 2, 3), (160, 48, 4, 10)]
INDEX = 7    # the camera of the orbit every single frame is rendered from


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
        c.set_kernel(hip.Context.PRODUCTION)
        c.set_scratch_fill(False)


@functools.lru_cache(maxsize=None)
def scene():
    return S.demo_scene(T.sky("synth"), anim_cameras([0], 160, 48)[0])


def kitty_text(rgb):
    """the host emitter's image text of a frame of bytes [rows, w, 3]"""
    rows, w, _ = rgb.shape
    text = host.emitter_kitty_rgb8(rgb)
    assert text.size == K.length(w, rows) == hip.kitty_bytes(w, rows)
    return text


@functools.lru_cache(maxsize=None)
def oracle(w, h, index, b, spp):
    """(the oracle's double frame, its bytes by the checker's cast, the emitter's image text of those) -- computed once, never written to"""
    px, _ = T.oracle_render(scene().with_camera(anim_cameras([index], w, h)[0]), w, h, b, spp)
    rgb = T.oracle_rgb8(px)
    text = kitty_text(rgb)
    px.flags.writeable = rgb.flags.writeable = text.flags.writeable = False
    return px, rgb, text


def device_kitty(ctx, cam, w, h, b, spp, offset=0, rows=None, what=""):
    rows = rows or hip.RowSet.whole(w, h)
    n = hip.kitty_bytes(w, owned_rows(rows))
    mem = DeviceBytes(n, offset)
    ctx.render_device_kitty(cam, rows, b, spp, mem.ptr, n)
    return mem.read(ctx, what)


def batch_kitty(ctx, cams, w, h, b, spp, offset=0, what=""):
    n = len(cams) * hip.kitty_bytes(w, h)
    mem = DeviceBytes(n, offset)
    ctx.render_batch_kitty(cams, hip.RowSet.whole(w, h), b, spp, mem.ptr, n)
    return mem.read(ctx, what).reshape(len(cams), -1)


def kitty_of_device_rgb8(ctx, rgb, offset=0, what=""):
    """trt_kitty_from_rgb8_device of a frame of bytes [rows, w, 3] uploaded at an odd address"""
    import torch
    rows, w, _ = rgb.shape
    src = torch.zeros(rgb.size + 1, dtype=torch.uint8, device="cuda:0")
    src[1:] = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1)).to("cuda:0")
    mem = DeviceBytes(hip.kitty_bytes(w, rows), offset)
    torch.cuda.synchronize()
    ctx.kitty_from_rgb8(src.data_ptr() + 1, w, rows, mem.ptr)
    return mem.read(ctx, what)


def same_text(got, want, what, rgb=None):
    """byte for byte the emitter's; and, where the frame is given, what the structural reader reads of it"""
    T.same_text(got, want, what)
    if rgb is not None:
        assert np.array_equal(K.read(np.asarray(got).tobytes()), rgb), what + ": the structural reader reads another frame"


# ---- 1. the wave's and the chunk's edges, at any alignment ----

def test_the_shapes_sit_on_the_edges():
    assert [w * h for w, h, _, _ in SHAPES] == [1, 63, 64, 65, 1023, 1024, 1025, 2049, 7680]
    assert hip.kitty_bytes(1, 1) == 60 and hip.kitty_bytes(160, 48) == 30846


@pytest.mark.parametrize("w,h,b,spp", SHAPES, ids=[f"{w}x{h}" for w, h, _, _ in SHAPES])
def test_any_alignment_with_a_filled_scratch_and_a_filled_output(ctx, w, h, b, spp):
    """trt_set_scratch_fill: the launch's samples and exactly its text bytes are 0xFF before the launch, so a sample the render kernel drops
    reads as 'AAAA' where the oracle's does not and a byte the pass skips stays 0xFF (no byte of a text is 0xFF); at every residue of the
    output address modulo the store's four bytes: the emitter's bytes, and not a byte outside them"""
    ctx.set_scratch_fill(True)
    ctx.set_scene(scene())
    cam = anim_cameras([INDEX], w, h)[0]
    _, rgb, want = oracle(w, h, INDEX, b, spp)
    assert not (want == 0xFF).any()
    for offset in range(STORE):
        same_text(device_kitty(ctx, cam, w, h, b, spp, offset, what=f"offset {offset}"), want, f"{w}x{h} at offset {offset}", rgb)


@pytest.mark.parametrize("w,h,b,spp", [SHAPES[3], SHAPES[6]], ids=["13x5", "41x25"])
def test_the_reference_order_kernel_goes_through_bytes(ctx, w, h, b, spp):
    ctx.set_kernel(hip.Context.REFERENCE_ORDER)
    ctx.set_scene(scene())
    cam = anim_cameras([INDEX], w, h)[0]
    _, rgb, want = oracle(w, h, INDEX, b, spp)
    for offset in (0, 3):
        same_text(device_kitty(ctx, cam, w, h, b, spp, offset, what="reference-order"), want, f"reference-order kernel, {w}x{h} at offset {offset}", rgb)


def test_a_shards_image_is_of_its_owned_rows_in_local_order(ctx):
    w, h, b, spp = 160, 48, 4, 10
    rows = hip.RowSet.shard(w, h, 1, 3, 2)  # tile_rows 2, tile_first 1, tile_step 3
    owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(owned_rows(rows))]
    assert 0 < len(owned) < h and owned[:4] == [2, 3, 8, 9]
    ctx.set_scene(scene())
    part = np.ascontiguousarray(oracle(w, h, INDEX, b, spp)[1][owned])
    got = device_kitty(ctx, anim_cameras([INDEX], w, h)[0], w, h, b, spp, offset=3, rows=rows, what="a shard")
    same_text(got, kitty_text(part), "a shard", part)
    assert b",s=00160,v=%05d," % len(owned) in got.tobytes()[:54]


# ---- 2. the frames of a batch start anywhere ----

@pytest.mark.parametrize("w,h", [(41, 25), (64, 32)], ids=["41x25", "64x32"])
def test_the_frames_of_a_batch_land_two_bytes_off_each_other(ctx, w, h):
    """K = 2: 4 P + 66 bytes, 2 modulo 4 -- from base offsets 0 and 1 the three frames start at residues 0, 2, 0 and 1, 3, 1; each is the
    single frame's text"""
    b, spp, indices = 2, 3, [7, 21, 33]
    n = hip.kitty_bytes(w, h)
    assert (w * h + 1023) // 1024 == 2 and n % STORE == 2
    ctx.set_scene(scene())
    cams = anim_cameras(indices, w, h)
    for offset in (0, 1):
        got = batch_kitty(ctx, cams, w, h, b, spp, offset, what=f"batch of 3 at offset {offset}")
        assert ctx.batch_info() == (3, 1)
        for k, index in enumerate(indices):
            _, rgb, want = oracle(w, h, index, b, spp)
            same_text(got[k], want, f"frame {k} of the batch at offset {offset}", rgb)
            single = device_kitty(ctx, cams[k], w, h, b, spp, (offset + k * n) % STORE, what="single")
            same_text(got[k], single, f"frame {k} of the batch against the single entry")


# ---- 3. host forms and the drop-in entry ----

def test_the_host_forms_and_the_drop_in_entry(ctx):
    w, h, b, spp = 160, 48, 4, 10
    rows = hip.RowSet.whole(w, h)
    indices = [7, 21]
    sc = scene()
    ctx.set_scene(sc)
    cams = anim_cameras(indices, w, h)
    wants = [oracle(w, h, i, b, spp) for i in indices]
    same_text(ctx.render_host_kitty(cams[0], rows, b, spp), wants[0][2], "render_host_kitty", wants[0][1])
    got = ctx.render_host_batch_kitty(cams, rows, b, spp)
    assert ctx.batch_info() == (2, 1)
    for k in range(2):
        same_text(got[k], wants[k][2], f"render_host_batch_kitty frame {k}", wants[k][1])
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    there = sc.with_camera(cams[1])
    same_text(hip.render_frame_kitty(there, w, h, b, spp), wants[1][2], "trt_render_frame_kitty", wants[1][1])
    same_text(hip.render_frame_kitty(there, w, h, b, spp), wants[1][2], "trt_render_frame_kitty, again")
    lib, text = hip.lib(), np.full(64, 0xA5, dtype=np.uint8)
    scene_struct = there.as_scene()
    assert lib.trt_render_frame_kitty(None, w, h, b, spp, text.ctypes.data) == ARGUMENT and lib.trt_render_frame_kitty(C.byref(scene_struct), w, h, b, spp, None) == ARGUMENT
    assert lib.trt_render_frame_kitty(C.byref(scene_struct), 100000, 1, b, spp, text.ctypes.data) == ARGUMENT
    assert lib.trt_render_frame_kitty(C.byref(scene_struct), 0, 1, b, spp, text.ctypes.data) == ARGUMENT and (text == 0xA5).all()
    hip._check(hip.lib().trt_shutdown())


# ---- 4. the formatting alone ----

@pytest.mark.parametrize("w,h", [(16, 16), (341, 3), (32, 32), (41, 25), (683, 3)], ids=lambda v: str(v))
def test_kitty_from_rgb8_formats_random_bytes_and_every_value_at_every_alignment(ctx, w, h):
    """P = 256 (every value of every channel too), 1023, 1024, 1025 and 2049 at offsets 0..3, into text bytes that held 0xA5: no render"""
    images = [np.random.default_rng(100 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)] + ([K.every_value_image()] if (w, h) == (16, 16) else [])
    for which, image in enumerate(images):
        want = kitty_text(image)
        for offset in range(STORE):
            same_text(kitty_of_device_rgb8(ctx, image, offset, what=f"image {which} at offset {offset}"), want, f"{w}x{h} image {which} at offset {offset}", image)


def test_kitty_from_rgb8_refuses_before_it_writes(ctx):
    mem = DeviceBytes(64)
    lib, p = hip.lib(), C.c_void_p(mem.ptr)
    call = lib.trt_kitty_from_rgb8_device
    assert call(None, p, 1, 1, p) == ARGUMENT and call(ctx._h, None, 1, 1, p) == ARGUMENT and call(ctx._h, p, 1, 1, None) == ARGUMENT
    assert call(ctx._h, p, 0, 1, p) == ARGUMENT and call(ctx._h, p, 1, -1, p) == ARGUMENT
    assert call(ctx._h, p, 100000, 1, p) == ARGUMENT and call(ctx._h, p, 1, 100000, p) == ARGUMENT
    assert mem.untouched(ctx)


# ---- 5. the queue ----

def test_a_kitty_frame_leaves_the_queue_ready_for_the_next_launch():
    """on one context: an image, doubles of the same shape, an image again -- a pass that did not arm the queue would hand the launch behind
    it a used-up one, and that launch would return a wrong frame with TRT_OK"""
    w, h, b, spp = 160, 48, 4, 10
    rows = hip.RowSet.whole(w, h)
    cams = anim_cameras([7, 21, 33], w, h)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    with hip.Context(0) as c:
        c.set_scene(scene())
        _, rgb, want = oracle(w, h, 7, b, spp)
        same_text(device_kitty(c, cams[0], w, h, b, spp, offset=1, what="first"), want, "the first image", rgb)
        assert np.array_equal(bits(c.render_host(cams[1], rows, b, spp)), bits(oracle(w, h, 21, b, spp)[0])), "doubles behind an image"
        _, rgb, want = oracle(w, h, 33, b, spp)
        same_text(device_kitty(c, cams[2], w, h, b, spp, offset=2, what="second"), want, "an image behind doubles", rgb)
        assert c.launch_count() == 3
        render_ms, reduce_ms = c.render_kernel_times()
        assert len(render_ms) == 3 and len(reduce_ms) == 3 and all(t > 0 for t in render_ms) and all(t > 0 for t in reduce_ms)


# ---- 6. the delta entries are undisturbed ----

def test_an_image_leaves_the_delta_entries_shown_frame_alone():
    w, h, b, spp = 41, 25, 2, 3
    rows = hip.RowSet.whole(w, h)
    cams = anim_cameras([7, 33], w, h)
    with hip.Context(0) as c:
        c.set_scene(scene())
        assert c.render_host_ansi_delta(cams[0], rows, b, spp).size == hip.ansi_bytes(w, h)  # a keyframe
        same_text(c.render_host_kitty(cams[1], rows, b, spp), oracle(w, h, 33, b, spp)[2], "the image of another camera")
        same_text(device_kitty(c, cams[1], w, h, b, spp, offset=1), oracle(w, h, 33, b, spp)[2], "the device entry")
        assert c.render_host_ansi_delta(cams[0], rows, b, spp).size == 0, "the shown frame changed under an image"


# ---- 7. errors, before anything is written ----

def test_refusals_enqueue_nothing_and_leave_the_context_rendering(ctx):
    lib = hip.lib()
    w, h, b, spp = 41, 25, 2, 3
    rows, bad_rows = hip.RowSet.whole(w, h), hip.RowSet(0, h, h, 0, 1)
    wide, tall = hip.RowSet.whole(100000, 1), hip.RowSet.whole(1, 100000)
    cams = anim_cameras([7, 21], w, h)
    cam = hip.camera_struct(cams[0])
    n = hip.kitty_bytes(w, h)
    mem = DeviceBytes(2 * n)
    text = np.full(2 * n, 0xA5, dtype=np.uint8)
    p, hp, cp, r = C.c_void_p(mem.ptr), C.c_void_p(text.ctypes.data), C.c_void_p(cams.ctypes.data), C.byref(rows)
    single = lambda c, camera=C.byref(cam), rs=r, bl=b, out=p, cap=n: lib.trt_render_device_kitty(c, camera, rs, bl, spp, out, cap)
    batch = lambda c, cameras=cp, k=2, rs=r, bl=b, out=p, cap=2 * n: lib.trt_render_device_batch_kitty(c, cameras, k, rs, bl, spp, out, cap)
    hsingle = lambda c, camera=C.byref(cam), rs=r, bl=b, out=hp: lib.trt_render_host_kitty(c, camera, rs, bl, spp, out)
    hbatch = lambda c, cameras=cp, k=2, rs=r, bl=b, out=hp: lib.trt_render_host_batch_kitty(c, cameras, k, rs, bl, spp, out)
    entries = (single, batch, hsingle, hbatch)
    with hip.Context(0) as empty:
        for entry in entries:
            assert entry(empty._h) == NO_SCENE
    ctx.set_scene(scene())
    h_ = ctx._h
    for entry in entries:
        refusals = [dict(c=None), dict(c=h_, out=None), dict(c=h_, rs=C.byref(bad_rows)), dict(c=h_, rs=None), dict(c=h_, bl=0),
                    dict(c=h_, rs=C.byref(wide)), dict(c=h_, rs=C.byref(tall))]
        refusals += [dict(c=h_, camera=None)] if entry in (single, hsingle) else [dict(c=h_, cameras=None), dict(c=h_, k=0), dict(c=h_, k=9)]
        for kw in refusals:
            kw = dict(kw, cap=1 << 40) if entry in (single, batch) else kw  # the limits are no matter of capacity
            assert entry(**kw) == ARGUMENT, sorted(kw)
    assert single(h_, cap=n - 1) == CAPACITY and batch(h_, cap=2 * n - 1) == CAPACITY
    assert mem.untouched(ctx), "a refused device entry wrote to the caller's buffer or its guards"
    assert (text == 0xA5).all(), "a refused host entry wrote to the caller's buffer"
    assert single(h_, cap=n) == 0  # to the byte
    same_text(mem.read(ctx)[:n], oracle(w, h, 7, b, spp)[2], "the good call after the refusals")
    assert batch(h_, cap=2 * n) == 0
    got = mem.read(ctx).reshape(2, n)
    for k, index in enumerate((7, 21)):
        same_text(got[k], oracle(w, h, index, b, spp)[2], f"the good batch after the refusals, frame {k}")
    same_text(ctx.render_host_batch_kitty(cams, rows, b, spp)[1], oracle(w, h, 21, b, spp)[2], "the host batch after the refusals")


# ---- 8. the demo ----

def test_demo_program_writes_one_image_per_frame(tmp_path):
    """examples/trt_demo --kitty: trt_render_frame_kitty into a buffer of trt_kitty_bytes, one fwrite per frame and nothing else on stdout --
    three texts of 30 846 bytes, each of which the structural reader takes for a 160 x 48 picture, the first the frame --rgb8 wrote"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    n = hip.kitty_bytes(160, 48)
    run = subprocess.run([exe, str(sky), "3", "160", "48", "--kitty", "--step=0.04"], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr[-500:]
    assert b"3 frames 160x48" in run.stderr and b"as a kitty image" in run.stderr
    assert len(run.stdout) == 3 * n
    frames = [K.read(run.stdout[k * n:(k + 1) * n]) for k in range(3)]
    assert all(f.shape == (48, 160, 3) for f in frames) and len(np.unique(frames[0].reshape(-1, 3), axis=0)) > 12, "a frame of one colour"
    quiet = subprocess.run([exe, str(sky), "3", "160", "48", "--kitty", "--no-draw"], capture_output=True, timeout=120)
    assert quiet.returncode == 0 and quiet.stdout == b"" and b"as a kitty image" in quiet.stderr, quiet.stderr[-500:]
    rgb8 = subprocess.run([exe, str(sky), "1", "160", "48", "--rgb8", "--step=0.04"], capture_output=True, timeout=120)
    assert rgb8.returncode == 0, rgb8.stderr[-500:]
    a = np.frombuffer(rgb8.stdout[:hip.ansi_bytes(160, 48)], dtype=np.uint8)[6:6 + (25 * 160 + 1) * 48].reshape(48, 25 * 160 + 1)[:, :25 * 160].reshape(48, 160, 25).astype(np.int32) - ord("0")
    first = np.stack([100 * a[..., at] + 10 * a[..., at + 1] + a[..., at + 2] for at in (7, 11, 15)], axis=-1).astype(np.uint8)
    assert np.array_equal(frames[0], first)
