"""The terminal's text written on the device (trt_render_device_ansi, trt_render_device_batch_ansi, trt_render_host_ansi,
trt_render_host_batch_ansi, trt_render_frame_ansi, trt_ansi_from_rgb8_device): behind the production kernel the pass that sums a pixel's
samples casts them to the emitter's bytes, formats the nine digits and stores the text itself, a wave per 384 aligned 32-bit words
(csrc/trt_ansi.h, trt_ansi.hpp).  The expected bytes never come from the library's text route: they are the host emitter's buffer
(host.Emitter(w, rows).patch_rgb8) of T.oracle_rgb8 -- the CPU checker's (int)(c*255) -- of the oracle's or the reference's double frame,
and the reference's own screenbuffer, tests/golden/emit_demo_160x48_b4.bin.z."""
import ctypes as C
import functools
import os
import subprocess
import zlib

import numpy as np
import pytest

import support as T
from support import STORE, DeviceBytes, anim_cameras, owned_rows, same_bytes, same_text
from terminalraytracer_amd import hip, host
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


def emitter_text(rgb):
    """the host emitter's buffer for a frame of bytes [rows, w, 3]: uint8 [8 + (25 w + 1) rows + 1]"""
    rows, w, _ = rgb.shape
    e = host.Emitter(w, rows)
    try:
        e.patch_rgb8(rgb)
        text = np.frombuffer(e.bytes(), dtype=np.uint8).copy()
    finally:
        e.close()
    assert text.size == 8 + (25 * w + 1) * rows + 1
    return text


@functools.lru_cache(maxsize=None)
def oracle(kind, w, h, index, b, spp):
    """(the oracle's double frame, its bytes by the checker's cast, the emitter's text of those, (path rays, shadow rays)) -- computed once, never
    written to"""
    px, st = T.oracle_render(scene(kind).with_camera(anim_cameras([index], w, h)[0]), w, h, b, spp)
    rgb = T.oracle_rgb8(px)
    text = emitter_text(rgb)
    px.flags.writeable = rgb.flags.writeable = text.flags.writeable = False
    return px, rgb, text, (st.path_rays, st.shadow_rays)


def device_ansi(ctx, cam, w, h, b, spp, offset=0, rows=None, what=""):
    rows = rows or hip.RowSet.whole(w, h)
    n = hip.ansi_bytes(w, owned_rows(rows))
    mem = DeviceBytes(n, offset)
    ctx.render_device_ansi(cam, rows, b, spp, mem.ptr, n)
    return mem.read(ctx, what)


def batch_ansi(ctx, cams, w, h, b, spp, offset=0, what=""):
    n = len(cams) * hip.ansi_bytes(w, h)
    mem = DeviceBytes(n, offset)
    ctx.render_batch_ansi(cams, hip.RowSet.whole(w, h), b, spp, mem.ptr, n)
    return mem.read(ctx, what).reshape(len(cams), -1)


def device_rgb8(ctx, cam, w, h, b, spp, offset=0):
    n = w * h * 3
    mem = DeviceBytes(n, offset)
    ctx.render_device_rgb8(cam, hip.RowSet.whole(w, h), b, spp, mem.ptr, n)
    return mem.read(ctx, "rgb8").reshape(h, w, 3)


def text_of_device_rgb8(ctx, rgb, offset=0, what=""):
    """trt_ansi_from_rgb8_device of a frame of bytes [rows, w, 3] uploaded at an odd address"""
    import torch
    rows, w, _ = rgb.shape
    src = torch.zeros(rgb.size + 1, dtype=torch.uint8, device="cuda:0")
    src[1:] = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1)).to("cuda:0")
    mem = DeviceBytes(hip.ansi_bytes(w, rows), offset)
    ctx.ansi_from_rgb8(src.data_ptr() + 1, w, rows, mem.ptr)
    return mem.read(ctx, what)


# ---- 1. the reference's bytes ----

def test_every_text_entry_gives_the_references_screenbuffer(ctx):
    """demo_160x48_b4: the 192 057 bytes the reference's buffered_draw_screen wrote, through the device entry, a batch of one, the host entry,
    trt_render_frame_ansi and trt_ansi_from_rgb8_device of the RGB8 entry's bytes"""
    name = "demo_160x48_b4"
    meta = T.golden_meta()["emitter"][name]
    case = next(c for c in T.golden_cases() if c["name"] == name)
    w, h, b, spp = case["width"], case["height"], case["bounce_limit"], case["rays_per_pixel"]
    with open(os.path.join(T.GOLDEN, "emit_demo_160x48_b4.bin.z"), "rb") as fh:
        want = np.frombuffer(zlib.decompress(fh.read()), dtype=np.uint8)
    assert want.size == meta["bytes"] == 192057 == hip.ansi_bytes(w, h) and T.fnv(want) == meta["fnv"]
    sc = T.golden_scene(case)
    ctx.set_scene(sc)
    rows = hip.RowSet.whole(w, h)
    routes = {"trt_render_device_ansi": device_ansi(ctx, sc.camera, w, h, b, spp, offset=1, what=name),
              "a batch of one": batch_ansi(ctx, np.array([sc.camera]), w, h, b, spp, offset=3, what=name)[0]}
    assert ctx.batch_info() == (1, 1)
    routes["trt_render_host_ansi"] = ctx.render_host_ansi(sc.camera, rows, b, spp)
    routes["trt_render_host_batch_ansi"] = ctx.render_host_batch_ansi(np.array([sc.camera]), rows, b, spp)[0]
    routes["trt_ansi_from_rgb8_device"] = text_of_device_rgb8(ctx, device_rgb8(ctx, sc.camera, w, h, b, spp), offset=2, what=name)
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    routes["trt_render_frame_ansi"] = hip.render_frame_ansi(sc, w, h, b, spp)
    for route, got in routes.items():
        same_text(got, want, f"{name} through {route}")
        assert T.fnv(got) == meta["fnv"], route


# ---- 2. any alignment, any size ----

SIZES = [(1, 1, 10), (1, 5, 3), (2, 3, 10), (3, 2, 1), (4, 3, 10), (7, 5, 10), (33, 3, 10), (63, 2, 3), (64, 1, 10), (65, 2, 10), (67, 13, 10)]


@pytest.mark.parametrize("w,h,spp", SIZES, ids=[f"{w}x{h}_spp{s}" for w, h, s in SIZES])
def test_any_alignment_and_any_size(ctx, w, h, spp):
    """a newline behind every cell (w = 1), row lengths 25 w + 1 of every residue modulo 4 (w = 1..4), a wave's 1536 bytes across several rows,
    rows that end around the end of a wave's span (w = 63, 64, 65: the first wave's span ends in cell 61 of row 0), several workgroups
    (67 x 13: 21 797 bytes, 15 waves) -- at every residue of the output address modulo the store's four bytes: the emitter's bytes, and not
    a byte outside them"""
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[2]
    for offset in range(STORE):
        same_text(device_ansi(ctx, cam, w, h, 4, spp, offset, what=f"offset {offset}"), want, f"{w}x{h} spp {spp} at offset {offset}")


# ---- 3. the frames of a batch start anywhere ----

def test_the_frames_of_a_batch_start_at_any_alignment(ctx):
    """three frames of 889 bytes from offset 1: they start 1, 890 and 1779 bytes behind an aligned address (residues 1, 2 and 3)"""
    w, h, indices = 7, 5, [7, 21, 33]
    assert hip.ansi_bytes(w, h) == 889
    ctx.set_scene(scene("demo"))
    cams = anim_cameras(indices, w, h)
    for spp in (10, 3):
        got = batch_ansi(ctx, cams, w, h, 4, spp, offset=1, what=f"batch of 3, spp {spp}")
        assert ctx.batch_info() == (3, 1)
        for k, index in enumerate(indices):
            same_text(got[k], oracle("demo", w, h, index, 4, spp)[2], f"frame {k} of the batch, spp {spp}")


ONE = [(67, 13, 3), (5, 1, 1)]  # 21 797 bytes, one more than a multiple of four: the text ends mid-word; 135 bytes: less than a wave's span


@pytest.mark.parametrize("w,h,spp", ONE, ids=[f"{w}x{h}_spp{s}" for w, h, s in ONE])
def test_a_batch_of_one_is_the_single_frame_entry_at_any_alignment(ctx, w, h, spp):
    """one camera through trt_render_device_batch_ansi and through trt_render_device_ansi at every residue of the output address: the same
    text, the emitter's, and not a byte outside it -- the two entries run ONE kernel, whose grid has exactly a single frame's waves"""
    assert hip.ansi_bytes(w, h) % STORE == 1 or hip.ansi_bytes(w, h) < 64 * STORE
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[2]
    for offset in range(STORE):
        single = device_ansi(ctx, cam, w, h, 4, spp, offset, what=f"single, offset {offset}")
        batch = batch_ansi(ctx, np.array([cam]), w, h, 4, spp, offset, what=f"batch of one, offset {offset}")
        assert ctx.batch_info() == (1, 1)
        same_text(batch[0], single, f"{w}x{h} spp {spp}: a batch of one against the single entry at offset {offset}")
        same_text(single, want, f"{w}x{h} spp {spp} at offset {offset}")


# ---- 4. every output kind on one context ----

def test_every_output_kind_interleaved_on_one_context():
    """doubles, bytes and text; single frames and batches; host and device entries, in turn, twice round: a queue that a text frame leaves
    unready for the next kind (or the reverse), a scratch sized for another kind or a history entry left open would show in a frame or in the
    count of kernel times"""
    w, h, b, spp = 160, 48, 4, 3
    rows = hip.RowSet.whole(w, h)
    indices = [0, 19, 59]
    cams = anim_cameras(indices, w, h)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    px, rgb, text = ([oracle("synth64", w, h, i, b, spp)[k] for i in indices] for k in range(3))
    with hip.Context(0) as c:
        c.set_scene(scene("synth64"))
        calls = 0
        for turn in range(2):
            assert np.array_equal(bits(c.render_host(cams[0], rows, b, spp)), bits(px[0])), turn
            same_text(c.render_host_ansi(cams[1], rows, b, spp), text[1], f"render_host_ansi, turn {turn}")
            same_bytes(c.render_host_rgb8(cams[2], rows, b, spp), rgb[2], f"render_host_rgb8 after text, turn {turn}")
            same_text(device_ansi(c, cams[2], w, h, b, spp, offset=turn + 1), text[2], f"render_device_ansi, turn {turn}")
            frames = c.render_host_batch(cams, rows, b, spp)
            for k in range(3):
                assert np.array_equal(bits(frames[k]), bits(px[k])), (turn, k)
            got = batch_ansi(c, cams, w, h, b, spp, offset=3 - turn)
            assert c.batch_info() == (3, 1)
            for k in range(3):
                same_text(got[k], text[k], f"render_batch_ansi frame {k}, turn {turn}")
            got = c.render_host_batch_rgb8(cams[::-1].copy(), rows, b, spp)
            for k in range(3):
                same_bytes(got[k], rgb[2 - k], f"render_host_batch_rgb8 after a text batch, frame {k}, turn {turn}")
            got = c.render_host_batch_ansi(cams[::-1].copy(), rows, b, spp)
            for k in range(3):
                same_text(got[k], text[2 - k], f"render_host_batch_ansi frame {k}, turn {turn}")
            assert np.array_equal(bits(c.render_host(cams[1], rows, b, spp)), bits(px[1])), ("doubles after a text batch", turn)
            calls += 9
            assert c.launch_count() == calls
        times = c.kernel_times()
        assert len(times) == calls and all(t > 0 for t in times)
        render_ms, reduce_ms = c.render_kernel_times()
        assert len(render_ms) == calls and len(reduce_ms) == calls and all(t > 0 for t in render_ms) and all(t > 0 for t in reduce_ms)


# ---- 5. the instantiations ----

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
def test_the_text_path_through_every_instantiation(ctx, setup):
    w, h, b, spp, index = 96, 32, 4, 3, 19
    kind, ran = setup(ctx)
    ctx.set_scene(scene(kind))
    cam = anim_cameras([index], w, h)[0]
    _, rgb, want, counts = oracle(kind, w, h, index, b, spp)
    same_text(device_ansi(ctx, cam, w, h, b, spp, offset=1, what=setup.__name__), want, setup.__name__ + ", device entry")
    assert ran(), setup.__name__
    if setup is _counting:
        assert ctx.read_counters() == counts
    same_text(ctx.render_host_ansi(cam, hip.RowSet.whole(w, h), b, spp), want, setup.__name__ + ", host entry")
    rows = hip.RowSet.shard(w, h, 1, 3, 4)
    owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(owned_rows(rows))]
    assert 0 < len(owned) < h
    same_text(device_ansi(ctx, cam, w, h, b, spp, offset=3, rows=rows), emitter_text(np.ascontiguousarray(rgb[owned])), setup.__name__ + ", a shard")


# ---- 6. filled scratch and filled output ----

def test_a_filled_scratch_and_a_filled_output_leave_the_emitters_text(ctx):
    """trt_set_scratch_fill: the launch's samples and exactly its text bytes are 0xFF before the launch -- a NaN in every double, which the cast
    turns into 0 and the text into 000 -- so a sample the render kernel drops prints 000 where the oracle does not, and a text byte the pass
    skips stays 0xFF; the bytes around the text keep their 0xA5"""
    ctx.set_scratch_fill(True)
    ctx.set_scene(scene("demo"))
    for w, h, spp in ((67, 13, 10), (7, 5, 3)):
        cam = anim_cameras([7], w, h)[0]
        _, rgb, want, _ = oracle("demo", w, h, 7, 4, spp)
        assert (rgb != 0).any() and not (want == 0xFF).any()
        for offset in (0, 3):
            same_text(device_ansi(ctx, cam, w, h, 4, spp, offset, what="filled"), want, f"filled, {w}x{h} at offset {offset}")
        same_text(ctx.render_host_ansi(cam, hip.RowSet.whole(w, h), 4, spp), want, f"filled, {w}x{h}, host entry")
    w, h, indices = 7, 5, [7, 21, 33]
    got = batch_ansi(ctx, anim_cameras(indices, w, h), w, h, 4, 3, offset=2, what="filled batch")
    for k, index in enumerate(indices):
        same_text(got[k], oracle("demo", w, h, index, 4, 3)[2], f"filled batch, frame {k}")
    ctx.set_kernel(hip.Context.REFERENCE_ORDER)
    same_text(device_ansi(ctx, anim_cameras([7], 7, 5)[0], 7, 5, 4, 3, offset=1, what="filled, reference-order"), oracle("demo", 7, 5, 7, 4, 3)[2],
              "filled, reference-order kernel")


# ---- 7. the formatting alone ----

def test_ansi_from_rgb8_formats_every_digit_triple_at_every_alignment(ctx):
    """a 16 x 16 image with r = i, g = 255 - i, b = 7 i mod 256: every value of every channel; a 5 x 3 image at offsets 0..3, into text bytes that
    held 0xFF"""
    i = np.arange(256)
    image = np.stack([i, 255 - i, (7 * i) & 255], axis=1).astype(np.uint8).reshape(16, 16, 3)
    for ch in range(3):
        assert len(set(image[..., ch].ravel())) == 256
    same_text(text_of_device_rgb8(ctx, image, offset=1, what="16 x 16"), emitter_text(image), "16 x 16, every digit triple")
    small = np.random.default_rng(5).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    for offset in range(STORE):
        same_text(text_of_device_rgb8(ctx, small, offset, what=f"5 x 3 at offset {offset}"), emitter_text(small), f"5 x 3 at offset {offset}")
    lib, p = hip.lib(), C.c_void_p(DeviceBytes(64).ptr)
    assert lib.trt_ansi_from_rgb8_device(None, p, 1, 1, p) == ARGUMENT and lib.trt_ansi_from_rgb8_device(ctx._h, None, 1, 1, p) == ARGUMENT
    assert lib.trt_ansi_from_rgb8_device(ctx._h, p, 1, 1, None) == ARGUMENT
    assert lib.trt_ansi_from_rgb8_device(ctx._h, p, 0, 1, p) == ARGUMENT and lib.trt_ansi_from_rgb8_device(ctx._h, p, 1, -1, p) == ARGUMENT


# ---- 8. errors ----

def test_refusals_enqueue_nothing_and_leave_the_context_rendering(ctx):
    import torch
    lib = hip.lib()
    w, h, b, spp = 33, 3, 4, 3
    rows, bad_rows = hip.RowSet.whole(w, h), hip.RowSet(0, h, h, 0, 1)
    cams = anim_cameras([7, 21], w, h)
    cam = hip.camera_struct(cams[0])
    n = hip.ansi_bytes(w, h)
    mem = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    text = np.full(2 * n, 0xA5, dtype=np.uint8)
    torch.cuda.synchronize()
    p, hp, cp, r = C.c_void_p(mem.data_ptr()), C.c_void_p(text.ctypes.data), C.c_void_p(cams.ctypes.data), C.byref(rows)
    with hip.Context(0) as empty:
        assert lib.trt_render_device_ansi(empty._h, C.byref(cam), r, b, spp, p, n) == NO_SCENE
        assert lib.trt_render_device_batch_ansi(empty._h, cp, 2, r, b, spp, p, 2 * n) == NO_SCENE
        assert lib.trt_render_host_batch_ansi(empty._h, cp, 2, r, b, spp, hp) == NO_SCENE
        assert lib.trt_render_host_ansi(empty._h, C.byref(cam), r, b, spp, hp) == NO_SCENE
    ctx.set_scene(scene("demo"))
    h_ = ctx._h
    single = lambda c=h_, camera=C.byref(cam), rs=r, bl=b, out=p, cap=n: lib.trt_render_device_ansi(c, camera, rs, bl, spp, out, cap)
    batch = lambda c=h_, cameras=cp, k=2, rs=r, bl=b, out=p, cap=2 * n: lib.trt_render_device_batch_ansi(c, cameras, k, rs, bl, spp, out, cap)
    hsingle = lambda c=h_, camera=C.byref(cam), rs=r, bl=b, out=hp: lib.trt_render_host_ansi(c, camera, rs, bl, spp, out)
    hbatch = lambda c=h_, cameras=cp, k=2, rs=r, bl=b, out=hp: lib.trt_render_host_batch_ansi(c, cameras, k, rs, bl, spp, out)
    for entry in (single, batch, hsingle, hbatch):
        assert entry(c=None) == ARGUMENT and entry(out=None) == ARGUMENT
        assert entry(rs=C.byref(bad_rows)) == ARGUMENT and entry(rs=None) == ARGUMENT
        assert entry(bl=0) == ARGUMENT
    assert single(camera=None) == ARGUMENT and hsingle(camera=None) == ARGUMENT
    other = cams.copy()
    other[1, 13] *= 2
    for entry in (batch, hbatch):
        assert entry(cameras=None) == ARGUMENT
        assert entry(k=0) == ARGUMENT and entry(k=9) == ARGUMENT
        assert entry(cameras=C.c_void_p(other.ctypes.data)) == ARGUMENT
    assert single(cap=n - 1) == CAPACITY and batch(cap=2 * n - 1) == CAPACITY
    ctx.synchronize()
    assert (mem.cpu().numpy() == 0xA5).all(), "a refused device entry wrote to the caller's buffer"
    assert single(cap=n) == 0 and batch(cap=2 * n) == 0  # to the byte
    ctx.synchronize()
    assert (text == 0xA5).all(), "a refused host entry wrote to the caller's buffer"
    got = mem.cpu().numpy().reshape(2, n)
    for k, index in enumerate((7, 21)):
        same_text(got[k], oracle("demo", w, h, index, 4, spp)[2], f"the good call after the refusals, frame {k}")
    same_text(ctx.render_host_batch_ansi(cams, rows, b, spp)[1], oracle("demo", w, h, 21, 4, spp)[2], "the host batch after the refusals")


# ---- 9. the demo ----

def test_demo_program_writes_the_devices_text(tmp_path):
    """examples/trt_demo --ansi: trt_render_frame_ansi into a buffer of trt_ansi_bytes, one fwrite, no emitter -- three texts of 192 057 bytes and
    the fps lines, the first of them what --rgb8 (bytes across PCIe, the host emitter) wrote for the same frame"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    n = hip.ansi_bytes(160, 48)
    # --step: frame k at orbit time 0.04 k in both runs (the wall clock's times differ from run to run)
    text = subprocess.run([exe, str(sky), "3", "160", "48", "--ansi", "--step=0.04"], capture_output=True, timeout=120)
    assert text.returncode == 0, text.stderr[-500:]
    assert b"3 frames 160x48" in text.stderr and b"as text" in text.stderr
    assert text.stdout.count(b"\033[48;2;") == 3 * 160 * 48 and text.stdout.count(b"\n\0\0\0") == 3
    assert len(text.stdout) >= 3 * n
    rgb8 = subprocess.run([exe, str(sky), "3", "160", "48", "--rgb8", "--step=0.04"], capture_output=True, timeout=120)
    assert rgb8.returncode == 0, rgb8.stderr[-500:]
    assert text.stdout[:n] == rgb8.stdout[:n] and text.stdout[n - 4:n] == b"\n\0\0\0"
    first = np.frombuffer(text.stdout[:n], dtype=np.uint8)
    assert len(set(first[6:].tobytes())) > 12, "a frame of one colour"
