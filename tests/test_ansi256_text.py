"""The terminal's texts in the xterm 256-colour palette written on the device (trt_render_device_ansi256[_half], the host and batch forms,
trt_render_frame_ansi256[_half], trt_ansi256[_half]_from_rgb8_device, trt_xterm256_from_rgb8_device): behind the production kernel the
pass that sums a pixel's samples casts them to the emitter's bytes, maps them to the palette by the closed form of csrc/trt_xterm256.h,
formats the index's digits and stores the text itself (csrc/trt_ansi256.hpp).  The expected bytes never come from the library's device
route: they are the sequential host emitters' (host.emitter_ansi256_rgb8, which finds its indices by the 240-entry search and which
tests/test_ansi256_layout.py reads back with a reader of its own) of the CPU checker's bytes of the oracle's frame, the frames
tests/stream_order_support.py computes once for every module that uses them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ansi256_support as A
import stream_order_support as O
import support as T
from support import owned_rows
from ansi256_support import DeviceBytes, same_text
from terminalraytracer_amd import hip, host

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4
W, SPP = O.W, O.SPP
KINDS = pytest.mark.parametrize("half", [False, True], ids=["full", "half_block"])


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
        c.set_scene_image(-1)
        c.set_compaction(-1)


def text_of(rgb, half):
    rows, w, _ = rgb.shape
    text = host.emitter_ansi256_rgb8(rgb, half)
    assert text.size == hip.ansi256_bytes(w, rows, half) == A.length(w, rows, half)
    return text


def device_text(ctx, cam, rows, b, half, offset=0, what=""):
    n = hip.ansi256_bytes(rows.width, owned_rows(rows), half)
    mem = DeviceBytes(n, offset)
    ctx.render_device_ansi256(cam, rows, b, SPP, mem.ptr, n, half)
    return mem.read(ctx, what)


# ---- 1. the palette map ----

def test_the_devices_palette_map_is_the_search_on_every_colour(ctx):
    """all 2^24 colours in one call against trt_xterm256_index_search's table; then seven pixels at an odd address into seven bytes at an odd
    address, with guards"""
    import torch
    want = A.search_table()
    c = torch.arange(1 << 24, dtype=torch.int32, device="cuda:0")
    rgb = torch.stack([c & 255, (c >> 8) & 255, c >> 16], dim=1).to(torch.uint8).contiguous()
    out = torch.zeros(1 << 24, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.xterm256_from_rgb8(rgb.data_ptr(), 1 << 24, out.data_ptr())
    ctx.synchronize()
    got = out.cpu().numpy()
    wrong = np.flatnonzero(got != want)
    assert wrong.size == 0, f"{wrong.size} colours differ, the first {wrong[0]:#08x}: {got[wrong[0]]} for {want[wrong[0]]}"
    assert got.min() == 16 and len(np.unique(got)) == 240
    seven = np.array([(0, 0, 0), (4, 4, 4), (5, 5, 5), (13, 13, 13), (47, 48, 115), (246, 246, 246), (247, 247, 247)], dtype=np.uint8)
    src, ptr = A.upload_odd(seven)
    mem = DeviceBytes(7, 3)
    assert ptr % 2 == 1 and mem.ptr % 4 == 3
    ctx.xterm256_from_rgb8(ptr, 7, mem.ptr)
    assert mem.read(ctx, "seven pixels").tolist() == [16, 16, 232, 232, 238, 255, 231]
    ctx.xterm256_from_rgb8(ptr, 0, mem.ptr)  # no pixel: nothing is written
    assert mem.read(ctx, "no pixel").tolist() == [16, 16, 232, 232, 238, 255, 231]
    lib, p = hip.lib(), C.c_void_p(mem.ptr)
    assert lib.trt_xterm256_from_rgb8_device(None, p, 1, p) == ARGUMENT and lib.trt_xterm256_from_rgb8_device(ctx._h, None, 1, p) == ARGUMENT
    assert lib.trt_xterm256_from_rgb8_device(ctx._h, p, 1, None) == ARGUMENT


# ---- 2. the formatting alone ----

@KINDS
@pytest.mark.parametrize("h", A.ROWS)
def test_formatting_alone_at_every_width_and_every_alignment(ctx, h, half):
    """the widths either side of the switch from rows shorter than a wave's span to longer ones, for both kinds, and of the lane's cell at
    width 64; random bytes and frames of tie and threshold colours only; every residue of the output address modulo the store's four bytes,
    guards either side; the last into memory that was never initialised"""
    for w in A.WIDTHS:
        for k, image in enumerate((np.random.default_rng(100 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8), A.edge_frame(w, h, w + h))):
            want = text_of(image, half)
            src, ptr = A.upload_odd(image)
            for offset in range(A.STORE):
                mem = DeviceBytes(want.size, offset, raw=offset == 3)
                ctx.ansi256_from_rgb8(ptr, w, h, mem.ptr, half)
                same_text(mem.read(ctx, f"{w}x{h}"), want, f"{w}x{h}, {'edge colours' if k else 'random bytes'}, offset {offset}")


# ---- 3. the fused routes ----

@KINDS
@pytest.mark.parametrize("route", list(O.ROUTES), ids=lambda r: r.replace(" ", "_"))
def test_the_fused_pass_on_every_route(ctx, route, half):
    """67 x 13 (an odd frame: 016 below the last row of the half-block text) and 67 x 12, device and host entries, and a shard whose owned
    rows are odd in number: the host emitter's text of the oracle's bytes"""
    r = O.ROUTES[route]
    O.configure(ctx, r)
    for h in (13, 12):
        frames = O.Frames(r.scene, r.bounce, h=h)
        rows = hip.RowSet.whole(W, h)
        rgb = frames.rgb(1)
        want = text_of(rgb, half)
        for offset in (1, 2):
            same_text(device_text(ctx, frames.camera(1), rows, r.bounce, half, offset, route), want, f"{route}, {W}x{h}, device entry at offset {offset}")
        same_text(ctx.render_host_ansi256(frames.camera(1), rows, r.bounce, SPP, half), want, f"{route}, {W}x{h}, host entry")
        if half and h % 2:
            assert want[-(23 * W + 5):].tobytes().count(b";48;5;016m") >= W
    frames = O.Frames(r.scene, r.bounce)
    shard = hip.RowSet.shard(W, O.HEIGHT, 0, 3, 1)
    owned = [hip.lib().trt_rowset_frame_row(C.byref(shard), i) for i in range(owned_rows(shard))]
    assert len(owned) % 2 == 1 and 1 < len(owned) < O.HEIGHT
    want = text_of(np.ascontiguousarray(frames.rgb(2)[owned]), half)
    same_text(device_text(ctx, frames.camera(2), shard, r.bounce, half, 3, route), want, f"{route}, a shard of {len(owned)} rows")
    same_text(ctx.render_host_ansi256(frames.camera(2), shard, r.bounce, SPP, half), want, f"{route}, a shard of {len(owned)} rows, host entry")


# ---- 4. a batch ----

@KINDS
def test_three_cameras_in_one_call_are_three_single_calls(ctx, half):
    r = O.ROUTES["plain rounds"]
    O.configure(ctx, r)
    frames = O.Frames(r.scene, r.bounce)
    rows = hip.RowSet.whole(W, O.HEIGHT)
    order = (2, 0, 3)
    cams = np.stack([frames.camera(c) for c in order])
    one = hip.ansi256_bytes(W, O.HEIGHT, half)
    singles = [device_text(ctx, frames.camera(c), rows, r.bounce, half, 1) for c in order]
    mem = DeviceBytes(3 * one, 3)
    ctx.render_batch_ansi256(cams, rows, r.bounce, SPP, mem.ptr, 3 * one, half)
    got = mem.read(ctx, "batch").reshape(3, one)
    assert ctx.batch_info() == (3, 1)  # three frames, one render launch
    on_host = ctx.render_host_batch_ansi256(cams, rows, r.bounce, SPP, half)
    assert ctx.batch_info() == (3, 1)
    for k, c in enumerate(order):
        same_text(got[k], singles[k], f"frame {k} of the batch against the single call")
        same_text(on_host[k], singles[k], f"frame {k} of the host batch against the single call")
        same_text(singles[k], text_of(frames.rgb(c), half), f"the single call of camera {c}")


# ---- 5. the delta entries are undisturbed ----

def test_a_delta_entry_before_and_after_still_returns_a_delta():
    r = O.ROUTES["plain rounds"]
    frames = O.Frames(r.scene, r.bounce)
    rows = hip.RowSet.whole(W, O.HEIGHT)
    with hip.Context(0) as c:
        O.configure(c, r)
        key = c.render_host_ansi_delta(frames.camera(0), rows, r.bounce, SPP)
        assert key.size == hip.ansi_bytes(W, O.HEIGHT)  # a keyframe
        for half in (False, True):
            same_text(c.render_host_ansi256(frames.camera(1), rows, r.bounce, SPP, half), text_of(frames.rgb(1), half), "another camera's frame")
            same_text(device_text(c, frames.camera(2), rows, r.bounce, half, 1), text_of(frames.rgb(2), half), "the device entry")
        assert c.render_host_ansi_delta(frames.camera(0), rows, r.bounce, SPP).size == 0, "the shown frame changed under a 256-colour frame"
        moved = c.render_host_ansi_delta(frames.camera(1), rows, r.bounce, SPP)
        assert 0 < moved.size < key.size and np.array_equal(moved, host.emitter_delta_rgb8(frames.rgb(0), frames.rgb(1)))


# ---- 6. the drop-in entries ----

@KINDS
def test_the_drop_in_entry_from_plain_host_structs(half):
    r = O.ROUTES["plain rounds"]
    frames = O.Frames(r.scene, r.bounce)
    sc = O.scene(r.scene).with_camera(frames.camera(3))
    want = text_of(frames.rgb(3), half)
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    same_text(hip.render_frame_ansi256(sc, W, O.HEIGHT, r.bounce, SPP, half), want, "trt_render_frame_ansi256" + ("_half" if half else ""))
    same_text(hip.render_frame_ansi256(sc, W, O.HEIGHT, r.bounce, SPP, half), want, "the same, again")
    lib, scene, out = hip.lib(), sc.as_scene(), np.zeros(want.size, dtype=np.uint8)
    entry = lib.trt_render_frame_ansi256_half if half else lib.trt_render_frame_ansi256
    assert entry(None, W, O.HEIGHT, r.bounce, SPP, out.ctypes.data) == ARGUMENT and entry(C.byref(scene), W, O.HEIGHT, r.bounce, SPP, None) == ARGUMENT
    assert entry(C.byref(scene), 0, O.HEIGHT, r.bounce, SPP, out.ctypes.data) == ARGUMENT and entry(C.byref(scene), W, 0, r.bounce, SPP, out.ctypes.data) == ARGUMENT
    assert not out.any()
    hip._check(hip.lib().trt_shutdown())


# ---- 7. errors ----

@KINDS
def test_refusals_enqueue_nothing_and_leave_the_context_rendering(ctx, half):
    import torch
    lib = hip.lib()
    r = O.ROUTES["plain rounds"]
    frames = O.Frames(r.scene, r.bounce)
    h, b = O.HEIGHT, r.bounce
    rows, no_rows = hip.RowSet.whole(W, h), hip.RowSet(W, 0, 1, 0, 1)
    assert owned_rows(no_rows) == 0
    cams = np.stack([frames.camera(0), frames.camera(1)])
    cam = hip.camera_struct(cams[0])
    n = hip.ansi256_bytes(W, h, half)
    mem = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    text = np.full(2 * n, 0xA5, dtype=np.uint8)
    torch.cuda.synchronize()
    p, hp, cp, rs = C.c_void_p(mem.data_ptr()), C.c_void_p(text.ctypes.data), C.c_void_p(cams.ctypes.data), C.byref(rows)
    name = lambda stem, mirror: getattr(lib, stem + ("_ansi_half" if mirror else "_ansi256_half" if half else "_ansi256"))
    pairs = []
    for mirror in (False, True):  # the entries and the _ansi_half entries they mirror: a refusal returns the same code
        single = lambda c, camera=C.byref(cam), rows=rs, bl=b, out=p, cap=n, f=name("trt_render_device", mirror): f(c, camera, rows, bl, SPP, out, cap)
        batch = lambda c, cameras=cp, k=2, rows=rs, bl=b, out=p, cap=2 * n, f=name("trt_render_device_batch", mirror): f(c, cameras, k, rows, bl, SPP, out, cap)
        hsingle = lambda c, camera=C.byref(cam), rows=rs, bl=b, out=hp, f=name("trt_render_host", mirror): f(c, camera, rows, bl, SPP, out)
        hbatch = lambda c, cameras=cp, k=2, rows=rs, bl=b, out=hp, f=name("trt_render_host_batch", mirror): f(c, cameras, k, rows, bl, SPP, out)
        pairs.append((single, batch, hsingle, hbatch))
    big = 1 << 30  # a capacity that holds either kind's text: the mirrors' texts are longer
    with hip.Context(0) as empty:
        for entry, mirror in zip(*pairs):
            kw = dict(cap=big) if entry in pairs[0][:2] else {}
            assert entry(empty._h, **kw) == mirror(empty._h, **kw) == NO_SCENE
    O.configure(ctx, r)
    h_ = ctx._h
    for entry, mirror in zip(*pairs):
        device = entry in pairs[0][:2]
        refusals = [dict(c=None), dict(c=h_, out=None), dict(c=h_, rows=C.byref(no_rows)), dict(c=h_, rows=None), dict(c=h_, bl=0)]
        refusals += [dict(c=h_, camera=None)] if entry in (pairs[0][0], pairs[0][2]) else [dict(c=h_, cameras=None), dict(c=h_, k=0), dict(c=h_, k=9)]
        for kw in refusals:
            if device:
                kw = dict(kw, cap=big)
            assert entry(**kw) == mirror(**kw) == ARGUMENT, sorted(kw)
    single, batch = pairs[0][:2]
    assert single(h_, cap=n - 1) == CAPACITY and batch(h_, cap=2 * n - 1) == CAPACITY
    from_rgb8 = lib.trt_ansi256_half_from_rgb8_device if half else lib.trt_ansi256_from_rgb8_device
    assert from_rgb8(None, p, 1, 1, p) == ARGUMENT and from_rgb8(h_, None, 1, 1, p) == ARGUMENT and from_rgb8(h_, p, 1, 1, None) == ARGUMENT
    assert from_rgb8(h_, p, 0, 1, p) == ARGUMENT and from_rgb8(h_, p, 1, 0, p) == ARGUMENT and from_rgb8(h_, p, 1, -1, p) == ARGUMENT
    ctx.synchronize()
    assert (mem.cpu().numpy() == 0xA5).all(), "a refused device entry wrote to the caller's buffer"
    assert (text == 0xA5).all(), "a refused host entry wrote to the caller's buffer"
    assert single(h_, cap=n) == 0 and batch(h_, cap=2 * n) == 0  # to the byte
    ctx.synchronize()
    got = mem.cpu().numpy().reshape(2, n)
    for k in range(2):
        same_text(got[k], text_of(frames.rgb(k), half), f"the good call after the refusals, frame {k}")
    same_text(ctx.render_host_ansi256(cams[0], rows, b, SPP, half), text_of(frames.rgb(0), half), "the host entry after the refusals")


# ---- 8. the demo ----

def test_demo_program_writes_the_devices_half_block_256_colour_text(tmp_path):
    """examples/trt_demo --256 --half: trt_render_frame_ansi256_half into a buffer of trt_ansi256_half_bytes, one fwrite per frame -- two texts
    of that length, each prefix, cells, row ends and nothing else"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    w, h = 67, 13
    n = hip.ansi256_bytes(w, h, True)
    run = subprocess.run([exe, str(sky), "2", str(w), str(h), "--256", "--half", "--step=0.04"], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr[-500:]
    assert b"2 frames 67x13" in run.stderr and b"as half-block 256-colour text" in run.stderr
    assert run.stdout.count(b"\xe2\x96\x80") == 2 * w * 7 and len(run.stdout) >= 2 * n
    first = A.read(run.stdout[:n], True)
    assert first.shape == (7, w, 2) and (first[-1, :, 1] == 16).all() and len(np.unique(first)) > 4, "a frame of one colour"
    refused = subprocess.run([exe, str(sky), "1", str(w), str(h), "--256", "--delta"], capture_output=True, timeout=120)
    assert refused.returncode == 2 and not refused.stdout
