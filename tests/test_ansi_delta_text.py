"""The delta text written on the device (trt_ansi_delta_from_rgb8_device, trt_render_device_ansi_delta, trt_render_host_ansi_delta,
trt_render_frame_ansi_delta, trt_ansi_delta_reset; csrc/trt_ansi_delta.h, trt_ansi_delta.hpp): three kernels place every changed cell's
record by a prefix sum over the frame.  The expected bytes never come from the device route: they are the sequential host statement
host.emitter_delta_rgb8 of pattern frames or of consecutive T.oracle_rgb8 frames, keyframes the host emitter's full text, and a model of a
terminal (ansi_delta_support.Terminal) must show every oracle frame after its text.  Every device buffer stands between guard bytes of 0xA5,
which also fill the text's room behind its length: none of them may change."""
import ctypes as C

import numpy as np
import pytest

import ansi_delta_support as D
import support as T
from ansi_delta_support import B, SPP, W, Room, at_odd_address, frames_of, same_text
from ansi_delta_support import HEIGHT as H
from terminalraytracer_amd import hip, host

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4


@pytest.fixture(scope="module")
def ctx():
    yield from D.fresh_context()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield from D.restore_defaults(request)


def device_delta(ctx, shown, nxt, offset=0, what=""):
    """with trap bytes behind each frame: a walk that loaded a cell behind the frame would see it changed"""
    return D.device_delta(ctx, hip.Context.ansi_delta_from_rgb8, hip.ansi_delta_capacity, shown, nxt, offset, what, trap=True)


# ---- 1. the formatting alone ----

SIZES = [(1, 1), (2, 1), (1, 3), (63, 2), (64, 1), (65, 3), (160, 48)]  # 160 x 48: 7.5 tiles of 1024 cells, the last one partial


@pytest.mark.parametrize("family", D.FAMILIES)
def test_the_formatting_alone_on_every_pattern_family(ctx, family):
    """one cell, one row, one column, rows around a wave's 256 cells, several tiles with a partial last one; the text at every residue of its address
    modulo 4 and both frames at odd addresses: length and bytes are the host's, nothing else is written, equal frames write nothing"""
    for w, rows in SIZES:
        shown, nxt = D.pair(family, w, rows)
        want = host.emitter_delta_rgb8(shown, nxt)
        for offset in range(4):
            same_text(device_delta(ctx, shown, nxt, offset, f"{family} {w}x{rows}"), want, f"{family} {w}x{rows} at offset {offset}")
        if family == "nothing":
            assert want.size == 0
        if family == "all different":
            assert want.size == D.bound(w, rows) <= hip.ansi_delta_capacity(w, rows)
    shown, _ = D.pair(family, 65, 3)
    assert device_delta(ctx, shown, shown.copy(), 1, "equal frames").size == 0


def test_more_tiles_than_one_turn_of_the_offsets_scan(ctx):
    """1920 x 1080: 2025 tiles, two turns of the one workgroup's 1024-sum scan with its running total; 40 % of the cells changed, and the longest
    text there is (every cell changed, all neighbours different: the bound, 43.6 MB)"""
    rng = np.random.default_rng(1080)
    w, rows = 1920, 1080
    shown = rng.integers(0, 256, (rows, w, 3), dtype=np.uint8)
    nxt = shown.copy()
    change = rng.random((rows, w)) < 0.4
    nxt[change] = rng.integers(0, 256, (int(change.sum()), 3), dtype=np.uint8)
    same_text(device_delta(ctx, shown, nxt, 3, "1080p, p = 0.4"), host.emitter_delta_rgb8(shown, nxt), "1080p, p = 0.4")
    nxt = shown ^ np.uint8(0x80)
    nxt[:, 1::2] ^= np.uint8(0x01)  # horizontal neighbours differ in the new frame wherever they were equal, and mostly anyway
    want = host.emitter_delta_rgb8(shown, nxt)
    same_text(device_delta(ctx, shown, nxt, 1, "1080p, everything changed"), want, "1080p, everything changed")
    assert want.size > 0.99 * D.bound(w, rows)


def test_the_formatting_entry_refuses_before_it_enqueues(ctx):
    lib = hip.lib()
    shown, nxt = D.pair("full palette 0.4", 7, 3)
    a, pa = at_odd_address(shown)
    b, pb = at_odd_address(nxt)
    cap = hip.ansi_delta_capacity(7, 3)
    assert cap == max(hip.ansi_bytes(7, 3), D.bound(7, 3)) and hip.ansi_delta_capacity(1, 1) == 39 and hip.ansi_delta_capacity(160, 48) == 192057
    assert hip.ansi_delta_capacity(49999, 1) == 8 + (25 * 49999 + 1) + 1 and hip.ansi_delta_capacity(1, 99999) == 39 * 99999
    assert hip.ansi_delta_capacity(50000, 1) == hip.ansi_delta_capacity(1, 100000) == hip.ansi_delta_capacity(0, 1) == hip.ansi_delta_capacity(1, -1) == 0
    room = Room(cap)
    call = lambda c=ctx._h, s=pa, n=pb, w=7, r=3, t=room.ptr, k=cap, l=room.length_ptr: lib.trt_ansi_delta_from_rgb8_device(c, s, n, w, r, t, k, l)
    for bad in (dict(c=None), dict(s=None), dict(n=None), dict(t=None), dict(l=None), dict(w=0), dict(r=0), dict(w=50000), dict(r=100000)):
        assert call(**bad) == ARGUMENT, bad
    assert call(k=cap - 1) == CAPACITY
    assert room.untouched(ctx)
    assert call() == 0
    same_text(room.text(ctx), host.emitter_delta_rgb8(shown, nxt), "the good call after the refusals")


# ---- 2. the render entries ----

render_delta = D.render_full


def check_sequence(ctx, scene_kind, rows, **more):
    D.check_sequence(D.FULL, ctx, scene_kind, rows, **more)


@pytest.mark.parametrize("kind", ["demo", "synth64"])
@pytest.mark.parametrize("kernel", [hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER], ids=["production", "reference_order"])
def test_a_keyframe_then_the_deltas_of_the_orbit(ctx, kind, kernel):
    ctx.set_scene(D.scene(kind))
    ctx.set_kernel(kernel)
    check_sequence(ctx, kind, hip.RowSet.whole(W, H), what=f"{kind} whole frame")
    ctx.ansi_delta_reset()
    check_sequence(ctx, kind, hip.RowSet(W, H, 8, 1, 3), what=f"{kind} shard")


def test_other_render_entries_leave_the_shown_frame_alone(ctx):
    """a trt_render_device_rgb8 and a trt_render_device_ansi call of another camera, and a trt_set_scene, between the delta calls"""
    import torch
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H)
    other = D.anim_cameras([40], W, H)[0]
    scratch = torch.zeros(hip.ansi_bytes(W, H), dtype=torch.uint8, device="cuda:0")

    def between(k):
        ctx.render_device_rgb8(other, rows, B, SPP, scratch.data_ptr(), W * H * 3)
        ctx.render_device_ansi(other, rows, B, SPP, scratch.data_ptr(), hip.ansi_bytes(W, H))
        if k == 1:
            ctx.set_scene(D.scene("demo"))

    check_sequence(ctx, "demo", rows, between=between, what="interleaved")


def test_reset_and_another_size_give_a_keyframe_and_the_host_entry_the_same_bytes(ctx):
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H)
    cams = D.anim_cameras([0, 1, 2, 3], W, H)
    f = frames_of("demo", [0, 1, 2, 3])
    same_text(ctx.render_host_ansi_delta(cams[0], rows, B, SPP), D.full_text(f[0]), "host entry, keyframe")
    same_text(ctx.render_host_ansi_delta(cams[1], rows, B, SPP), host.emitter_delta_rgb8(f[0], f[1]), "host entry, delta")
    same_text(render_delta(ctx, cams[2], rows, 1), host.emitter_delta_rgb8(f[1], f[2]), "device entry after the host entry")
    ctx.ansi_delta_reset()
    same_text(render_delta(ctx, cams[3], rows, 2), D.full_text(f[3]), "after trt_ansi_delta_reset")
    same_text(ctx.render_host_ansi_delta(cams[3], rows, B, SPP), np.zeros(0, dtype=np.uint8), "the same frame again")
    shard = hip.RowSet(W, H, 8, 1, 3)
    same_text(ctx.render_host_ansi_delta(cams[2], shard, B, SPP), D.full_text(frames_of("demo", [2], shard)[0]), "another rowset")
    same_text(render_delta(ctx, cams[2], rows, 3), D.full_text(f[2]), "and back: the whole frame is no longer the shown one")
    small = hip.RowSet.whole(33, 3)
    got = ctx.render_host_ansi_delta(D.anim_cameras([7], 33, 3)[0], small, B, 3)
    same_text(got, D.full_text(T.oracle_rgb8(T.oracle_render(D.scene("demo").with_camera(D.anim_cameras([7], 33, 3)[0]), 33, 3, B, 3)[0])), "another size")


def test_refusals_keep_the_shown_frame(ctx):
    lib = hip.lib()
    rows, bad_rows, wide = hip.RowSet.whole(W, H), hip.RowSet(0, H, H, 0, 1), hip.RowSet.whole(50000, 1)
    cams = D.anim_cameras([0, 1, 2], W, H)
    f = frames_of("demo", [0, 1, 2])
    cam = [hip.camera_struct(c) for c in cams]
    cap = hip.ansi_delta_capacity(W, H)
    room = Room(max(cap, hip.ansi_delta_capacity(49999, 1)))
    text = np.full(room.capacity, 0xA5, dtype=np.uint8)
    n = C.c_size_t(77)
    with hip.Context(0) as empty:
        assert lib.trt_render_device_ansi_delta(empty._h, C.byref(cam[0]), C.byref(rows), B, SPP, room.ptr, cap, room.length_ptr) == NO_SCENE
        assert lib.trt_render_host_ansi_delta(empty._h, C.byref(cam[0]), C.byref(rows), B, SPP, text.ctypes.data, cap, C.byref(n)) == NO_SCENE
        empty.set_scene(D.scene("demo"))
        same_text(empty.render_host_ansi_delta(cams[0], rows, B, SPP), D.full_text(f[0]), "a good call after no scene")
    ctx.set_scene(D.scene("demo"))
    same_text(render_delta(ctx, cams[0], rows), D.full_text(f[0]), "keyframe")
    device = lambda c=ctx._h, camera=C.byref(cam[1]), rs=C.byref(rows), bl=B, out=room.ptr, k=cap, l=room.length_ptr: \
        lib.trt_render_device_ansi_delta(c, camera, rs, bl, SPP, out, k, l)
    hosted = lambda c=ctx._h, camera=C.byref(cam[1]), rs=C.byref(rows), bl=B, out=text.ctypes.data, k=cap, l=C.byref(n): \
        lib.trt_render_host_ansi_delta(c, camera, rs, bl, SPP, out, k, l)
    for entry in (device, hosted):
        for bad in (dict(c=None), dict(camera=None), dict(rs=None), dict(out=None), dict(l=None), dict(rs=C.byref(bad_rows)), dict(bl=0),
                    dict(rs=C.byref(wide), k=room.capacity)):
            assert entry(**bad) == ARGUMENT, bad
        assert entry(k=cap - 1) == CAPACITY
    assert room.untouched(ctx), "a refused device entry wrote to the caller's buffer"
    assert (text == 0xA5).all() and n.value == 77, "a refused host entry wrote to the caller's buffer"
    same_text(render_delta(ctx, cams[1], rows, 1), host.emitter_delta_rgb8(f[0], f[1]), "the good call after the refusals is still a delta")
    assert hosted(camera=C.byref(cam[2])) == 0
    same_text(text[:n.value], host.emitter_delta_rgb8(f[1], f[2]), "and so is the host entry's")
    assert (text[n.value:] == 0xA5).all()


# ---- 3. the drop-in entry ----

def test_the_default_contexts_entry(ctx):
    """keyframe, delta, a sphere moved between two calls (the delta is between the two frames whatever changed), trt_shutdown, keyframe"""
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    cams = D.anim_cameras([0, 1, 2], W, H)
    base = D.scene("demo")
    f0, f1 = frames_of("demo", [0, 1])
    f2 = D.oracle_rgb("demo", "synth", W, H, 2, B, SPP, moved=True)
    term = D.Terminal(W, H)
    try:
        got = hip.render_frame_ansi_delta(base.with_camera(cams[0]), W, H, B, SPP)
        same_text(got, D.full_text(f0), "keyframe")
        term.feed(got).shows(f0, "keyframe")
        got = hip.render_frame_ansi_delta(base.with_camera(cams[1]), W, H, B, SPP)
        same_text(got, host.emitter_delta_rgb8(f0, f1), "delta")
        term.feed(got).shows(f1, "delta")
        got = hip.render_frame_ansi_delta(D.moved_scene(base.with_camera(cams[2])), W, H, B, SPP)
        same_text(got, host.emitter_delta_rgb8(f1, f2), "a sphere moved")
        term.feed(got).shows(f2, "a sphere moved")
        assert (f2 != D.oracle_rgb("demo", "synth", W, H, 2, B, SPP)).any()
        hip._check(hip.lib().trt_shutdown())
        same_text(hip.render_frame_ansi_delta(base.with_camera(cams[1]), W, H, B, SPP), D.full_text(f1), "keyframe after trt_shutdown")
        lib, scene, n = hip.lib(), base.as_scene(), C.c_size_t(0)
        out = np.full(hip.ansi_delta_capacity(W, H), 0xA5, dtype=np.uint8)
        assert lib.trt_render_frame_ansi_delta(None, W, H, B, SPP, out.ctypes.data, out.size, C.byref(n)) == ARGUMENT
        assert lib.trt_render_frame_ansi_delta(C.byref(scene), W, H, B, SPP, None, out.size, C.byref(n)) == ARGUMENT
        assert lib.trt_render_frame_ansi_delta(C.byref(scene), W, H, B, SPP, out.ctypes.data, out.size, None) == ARGUMENT
        assert lib.trt_render_frame_ansi_delta(C.byref(scene), 50000, 1, B, SPP, out.ctypes.data, out.size, C.byref(n)) == ARGUMENT
        assert lib.trt_render_frame_ansi_delta(C.byref(scene), W, H, B, SPP, out.ctypes.data, out.size - 1, C.byref(n)) == CAPACITY
        assert (out == 0xA5).all()
    finally:
        hip._check(hip.lib().trt_shutdown())


# ---- 4. the demo ----

def test_demo_program_draws_the_orbit_from_a_keyframe_and_deltas(tmp_path):
    """examples/trt_demo --delta: the keyframe and three delta texts on stdout and nothing else -- the fps line goes to stderr -- leave the terminal
    with the picture that --ansi's last whole text of the same replay paints"""
    import os
    import subprocess
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    n = hip.ansi_bytes(W, H)
    delta = subprocess.run([exe, str(sky), "4", str(W), str(H), "--delta", "--step=0.0166667"], capture_output=True, timeout=120)
    assert delta.returncode == 0, delta.stderr[-500:]
    assert b"4 frames 160x48" in delta.stderr and b"as delta text" in delta.stderr and b" fps, " in delta.stderr
    assert n < len(delta.stdout) < n + 3 * 0.84 * n and delta.stdout[n - 4:n] == b"\n\0\0\0"
    whole = subprocess.run([exe, str(sky), "4", str(W), str(H), "--ansi", "--step=0.0166667"], capture_output=True, timeout=120)
    assert whole.returncode == 0, whole.stderr[-500:]
    assert delta.stdout[:n] == whole.stdout[:n]
    last = whole.stdout.rindex(b"\033[0;0H\033[48;2;")
    want = D.Terminal(W, H).feed(whole.stdout[last:last + n])
    got = D.Terminal(W, H).feed(delta.stdout)
    assert (want.grid >= 0).all() and np.array_equal(got.grid, want.grid)
