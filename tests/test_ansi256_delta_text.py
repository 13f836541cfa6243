"""The delta texts in the xterm 256-colour palette written on the device, in full cells and in half-block cells
(trt_ansi256_delta[_half]_from_rgb8_device, trt_render_device_ansi256_delta[_half], trt_render_host_ansi256_delta[_half],
trt_render_frame_ansi256_delta[_half]; csrc/trt_ansi256_delta.h, trt_ansi256_delta_half.h, trt_ansi_delta.hpp): the three kernels of the
24-bit delta texts, whose walk maps the RGB8 bytes it loads to palette entries and compares those.  The expected bytes never come from the
device route: they are the sequential host statement host.emitter_delta256_rgb8 -- which SEARCHES the palette -- of pattern frames or of
consecutive T.oracle_rgb8 frames, keyframes host.emitter_ansi256_rgb8's text, and a model of a terminal
(ansi256_delta_support.Terminal, HalfTerminal) must show every oracle frame's entries after its text.  Every device buffer stands between
guard bytes of 0xA5, which also fill the text's room behind its length: none of them may change."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import ansi256_delta_support as A
import ansi_delta_support as D
import support as T
from ansi_delta_support import B, SPP, W, Room, at_odd_address, frames_of, same_text
from ansi_delta_support import HEIGHT as H_
from terminalraytracer_amd import hip, host

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4
KIND_IDS = sorted(A.KINDS)


def is_half(kind):
    return kind.startswith("half")


@pytest.fixture(scope="module")
def ctx():
    yield from D.fresh_context()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield from D.restore_defaults(request)


def device_delta(ctx, kind, shown, nxt, offset=0, what="", trap=False):
    k = A.KINDS[kind]
    return D.device_delta(ctx, k.single, k.capacity, shown, nxt, offset, what, trap)


# ---- 1. the formatting alone ----

SIZES = [(67, 13), (131, 17)]  # 131 x 17: rows that straddle the tiles' edges (full cells: three tiles; half-block cells: two, an odd last row)
SMALL = [(1, 1), (2, 1), (3, 2)]


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_formatting_alone_on_every_pattern_family(ctx, kind):
    """every family of the 24-bit delta texts and the three of the palette's, frames at odd addresses, the text at the residues of its
    address modulo 4 in turn: length and bytes are the host's, nothing else is written"""
    half, k = is_half(kind), A.KINDS[kind]
    for n, (family, (w, rows)) in enumerate(itertools.product(A.HALF_FAMILIES if half else A.FAMILIES, SIZES)):
        shown, nxt = A.pair(family, w, rows, half=half)
        want = k.delta(shown, nxt)
        same_text(device_delta(ctx, kind, shown, nxt, n % 4, f"{family} {w}x{rows}", trap=True), want, f"{kind} {family} {w}x{rows}")
        if family in ("nothing", "same index"):
            assert want.size == 0
        if family == "longest" and not (half and rows % 2):
            assert want.size == A.bound(w, rows, half) == k.capacity(w, rows)


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_smallest_screens_and_a_room_of_exactly_the_capacity(ctx, kind):
    """1 x 1, 2 x 1 and 3 x 2 in the family that fills the room to its last byte; one byte less is TRT_ERR_CAPACITY with nothing stored"""
    half, k = is_half(kind), A.KINDS[kind]
    for w, rows in SMALL:
        for family in ("longest", "index run", "same index", "all different", "last only"):
            shown, nxt = A.pair(family, w, rows, half=half)
            for offset in range(4):
                same_text(device_delta(ctx, kind, shown, nxt, offset, f"{family} {w}x{rows}", trap=True), k.delta(shown, nxt), f"{kind} {family} {w}x{rows} at offset {offset}")
        shown, nxt = A.pair("longest", w, rows, half=half)
        cap = k.capacity(w, rows)
        assert cap == A.bound(w, rows, half) and (half and rows % 2 or k.delta(shown, nxt).size == cap)
        a, pa = at_odd_address(shown)
        b, pb = at_odd_address(nxt)
        room = Room(cap, 1)
        entry = getattr(hip.lib(), "trt_ansi256_delta" + ("_half" if half else "") + "_from_rgb8_device")
        assert entry(ctx._h, pa, pb, w, rows, room.ptr, cap - 1, room.length_ptr) == CAPACITY
        assert room.untouched(ctx)
        assert entry(ctx._h, pa, pb, w, rows, room.ptr, cap, room.length_ptr) == 0
        same_text(room.text(ctx), k.delta(shown, nxt), f"{kind} {w}x{rows} in a room of exactly the capacity")
    assert hip.ansi256_delta_capacity(1, 1) == 31 and hip.ansi256_delta_capacity(2, 1) == 44 and hip.ansi256_delta_capacity(1, 1, half=True) == 41


@pytest.mark.parametrize("family", ["nothing", "all different", "full palette 0.4", "upper only", "longest", "same index"])
def test_nothing_behind_an_odd_half_block_frame_is_read(ctx, family):
    """odd frames, each followed directly by width * 3 bytes that differ between the two allocations -- black behind `shown`, white behind
    `next`, other entries -- : a kernel that loaded a lower row there would see changed cells; the text is still the host's"""
    for w, rows in [(1, 1), (2, 1), (65, 5), (131, 17)]:
        shown, nxt = A.pair(family, w, rows, half=True)
        same_text(device_delta(ctx, "half256", shown, nxt, 1, f"{family} {w}x{rows}", trap=True), host.emitter_delta256_rgb8(shown, nxt, half=True),
                  f"{family} {w}x{rows} with a trap row")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_more_tiles_than_one_turn_of_the_offsets_scan(ctx, kind):
    """1025 x 1025: 1027 tiles of full cells -- two turns of the one workgroup's 1024-sum scan with its running total -- and 514 of half-block
    cells, an odd frame; 1 % of the pixels changed"""
    half = is_half(kind)
    shown, nxt = A.pair("full palette 0.01", 1025, 1025, half=half)
    tiles = -(-1025 * ((1025 + 1) // 2 if half else 1025) // 1024)
    assert tiles == (514 if half else 1027)
    same_text(device_delta(ctx, kind, shown, nxt, 3, "1025x1025", trap=True), A.KINDS[kind].delta(shown, nxt), f"{kind} 1025x1025, p = 0.01")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_formatting_entry_refuses_before_it_enqueues(ctx, kind):
    half, k, lib = is_half(kind), A.KINDS[kind], hip.lib()
    entry = getattr(lib, "trt_ansi256_delta" + ("_half" if half else "") + "_from_rgb8_device")
    shown, nxt = A.pair("full palette 0.4", 7, 3, half=half)
    a, pa = at_odd_address(shown)
    b, pb = at_odd_address(nxt)
    cap = k.capacity(7, 3)
    assert cap == max(hip.ansi256_bytes(7, 3, half=half), A.bound(7, 3, half))
    too_wide, too_high = (100000, 199999) if half else (50000, 100000)
    assert k.capacity(too_wide, 1) == k.capacity(1, too_high) == k.capacity(0, 1) == k.capacity(1, 0) == k.capacity(-1, 1) == 0
    assert k.capacity(too_wide - 1, 1) > 0 and k.capacity(1, too_high - 1) > 0
    room = Room(cap)
    call = lambda c=ctx._h, s=pa, n=pb, w=7, r=3, t=room.ptr, cp=cap, l=room.length_ptr: entry(c, s, n, w, r, t, cp, l)
    for bad in (dict(c=None), dict(s=None), dict(n=None), dict(t=None), dict(l=None), dict(w=0), dict(r=0), dict(w=too_wide, cp=1 << 40), dict(r=too_high, cp=1 << 40)):
        assert call(**bad) == ARGUMENT, bad
    assert call(cp=cap - 1) == CAPACITY
    assert room.untouched(ctx)
    assert call() == 0
    same_text(room.text(ctx), k.delta(shown, nxt), "the good call after the refusals")
    ms = ctx.ansi256_delta_kernel_times(pa, pb, 7, 3, room.ptr, cap, room.length_ptr, half=half)
    assert len(ms) == 3 and all(t >= 0 for t in ms)
    same_text(room.text(ctx), k.delta(shown, nxt), "the timing entry writes the same text")


# ---- 2. the render entries ----

@pytest.mark.parametrize("scene_kind", ["demo", "synth64"])
@pytest.mark.parametrize("kernel", [hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER], ids=["production", "reference_order"])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_keyframe_then_the_deltas_of_the_orbit(ctx, kind, kernel, scene_kind):
    """a keyframe and the deltas of four frames: each text is the emitter's of the oracle's frames, the fed terminal shows each frame's entries"""
    ctx.set_scene(D.scene(scene_kind))
    ctx.set_kernel(kernel)
    D.check_sequence(A.KINDS[kind], ctx, scene_kind, hip.RowSet.whole(W, H_), indices=(0, 1, 2, 3, 4), what=f"{kind} {scene_kind} whole frame")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_an_odd_frame_and_a_sharded_rowset(ctx, kind):
    """160 x 47: the last text row's lower halves are the palette's black in every half-block text; a shard's rows count from its first one"""
    ctx.set_scene(D.scene("demo"))
    D.check_sequence(A.KINDS[kind], ctx, "demo", hip.RowSet.whole(W, 47), what=f"{kind} demo 160x47", h=47)
    ctx.ansi_delta_reset()
    D.check_sequence(A.KINDS[kind], ctx, "demo", hip.RowSet(W, H_, 8, 1, 3), what=f"{kind} demo shard")


def test_the_shown_frame_across_all_four_kinds(ctx):
    """every ordered pair of different kinds: a call of kind b behind a call of kind a is b's keyframe; staying within a kind is a delta.  The
    existing pairs, full and half-block cells in 24-bit colour, give what they gave before there were four"""
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H_)
    cams, f = D.anim_cameras(range(4), W, H_), frames_of("demo", range(4))
    for a, b in itertools.permutations(sorted(A.ALL_KINDS), 2):
        ka, kb = A.ALL_KINDS[a], A.ALL_KINDS[b]
        ctx.ansi_delta_reset()
        same_text(ka.render(ctx, cams[0], rows), ka.keyframe(f[0]), f"{a}: keyframe")
        same_text(ka.render(ctx, cams[1], rows, offset=1), ka.delta(f[0], f[1]), f"{a}: staying within the kind is a delta")
        same_text(kb.render(ctx, cams[2], rows, offset=2), kb.keyframe(f[2]), f"{b} behind {a}: a keyframe")
        same_text(kb.render(ctx, cams[3], rows, offset=3), kb.delta(f[2], f[3]), f"{b} behind {a}: then a delta")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_other_entries_leave_the_shown_frame_alone(ctx, kind):
    """the whole-text entries of every kind, the RGB8 and the sixel entry of another camera, and a trt_set_scene, between the delta calls"""
    import torch
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H_)
    other = D.anim_cameras([40], W, H_)[0]
    scratch = torch.zeros(max(hip.ansi_bytes(W, H_), hip.sixel_capacity(W, H_)), dtype=torch.uint8, device="cuda:0")
    length = torch.zeros(1, dtype=torch.int64, device="cuda:0")

    def between(k):
        ctx.render_device_rgb8(other, rows, B, SPP, scratch.data_ptr(), W * H_ * 3)
        ctx.render_device_ansi(other, rows, B, SPP, scratch.data_ptr(), hip.ansi_bytes(W, H_))
        ctx.render_device_ansi_half(other, rows, B, SPP, scratch.data_ptr(), hip.ansi_half_bytes(W, H_))
        for half in (False, True):
            ctx.render_device_ansi256(other, rows, B, SPP, scratch.data_ptr(), hip.ansi256_bytes(W, H_, half=half), half=half)
        ctx.render_device_sixel(other, rows, B, SPP, scratch.data_ptr(), hip.sixel_capacity(W, H_), length.data_ptr())
        if k == 1:
            ctx.set_scene(D.scene("demo"))

    D.check_sequence(A.KINDS[kind], ctx, "demo", rows, between=between, what=f"{kind} interleaved")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_reset_and_another_size_give_a_keyframe_and_the_host_entry_the_same_bytes(ctx, kind):
    half, k = is_half(kind), A.KINDS[kind]
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H_)
    cams, f = D.anim_cameras([0, 1, 2, 3], W, H_), frames_of("demo", [0, 1, 2, 3])
    hosted = lambda cam, rs=rows, spp=SPP: ctx.render_host_ansi256_delta(cam, rs, B, spp, half=half)
    same_text(hosted(cams[0]), k.keyframe(f[0]), "host entry, keyframe")
    same_text(hosted(cams[1]), k.delta(f[0], f[1]), "host entry, delta")
    same_text(k.render(ctx, cams[2], rows, offset=1), k.delta(f[1], f[2]), "device entry after the host entry")
    ctx.ansi_delta_reset()
    same_text(k.render(ctx, cams[3], rows, offset=2), k.keyframe(f[3]), "after trt_ansi_delta_reset")
    same_text(hosted(cams[3]), np.zeros(0, dtype=np.uint8), "the same frame again")
    shard = hip.RowSet(W, H_, 8, 1, 3)
    same_text(hosted(cams[2], shard), k.keyframe(frames_of("demo", [2], shard)[0]), "another rowset")
    same_text(k.render(ctx, cams[2], rows, offset=3), k.keyframe(f[2]), "and back: the whole frame is no longer the shown one")
    small, cam = hip.RowSet.whole(33, 3), D.anim_cameras([7], 33, 3)[0]
    same_text(hosted(cam, small, 3), k.keyframe(T.oracle_rgb8(T.oracle_render(D.scene("demo").with_camera(cam), 33, 3, B, 3)[0])), "another size")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_refusals_keep_the_shown_frame(ctx, kind):
    half, k, lib = is_half(kind), A.KINDS[kind], hip.lib()
    suffix = "_half" if half else ""
    device_entry, host_entry = getattr(lib, "trt_render_device_ansi256_delta" + suffix), getattr(lib, "trt_render_host_ansi256_delta" + suffix)
    rows, bad_rows, wide = hip.RowSet.whole(W, H_), hip.RowSet(0, H_, H_, 0, 1), hip.RowSet.whole(100000, 1)
    cams, f = D.anim_cameras([0, 1, 2], W, H_), frames_of("demo", [0, 1, 2])
    cam = [hip.camera_struct(c) for c in cams]
    cap = k.capacity(W, H_)
    room = Room(max(cap, k.capacity(49999, 1)))
    text = np.full(room.capacity, 0xA5, dtype=np.uint8)
    n = C.c_size_t(77)
    with hip.Context(0) as empty:
        assert device_entry(empty._h, C.byref(cam[0]), C.byref(rows), B, SPP, room.ptr, cap, room.length_ptr) == NO_SCENE
        assert host_entry(empty._h, C.byref(cam[0]), C.byref(rows), B, SPP, text.ctypes.data, cap, C.byref(n)) == NO_SCENE
    ctx.set_scene(D.scene("demo"))
    same_text(k.render(ctx, cams[0], rows), k.keyframe(f[0]), "keyframe")
    device = lambda c=ctx._h, camera=C.byref(cam[1]), rs=C.byref(rows), bl=B, out=room.ptr, cp=cap, l=room.length_ptr: device_entry(c, camera, rs, bl, SPP, out, cp, l)
    hosted = lambda c=ctx._h, camera=C.byref(cam[1]), rs=C.byref(rows), bl=B, out=text.ctypes.data, cp=cap, l=C.byref(n): host_entry(c, camera, rs, bl, SPP, out, cp, l)
    for entry in (device, hosted):
        for bad in (dict(c=None), dict(camera=None), dict(rs=None), dict(out=None), dict(l=None), dict(rs=C.byref(bad_rows)), dict(bl=0),
                    dict(rs=C.byref(wide), cp=room.capacity)):
            assert entry(**bad) == ARGUMENT, bad
        assert entry(cp=cap - 1) == CAPACITY
    assert room.untouched(ctx), "a refused device entry wrote to the caller's buffer"
    assert (text == 0xA5).all() and n.value == 77, "a refused host entry wrote to the caller's buffer"
    same_text(k.render(ctx, cams[1], rows, offset=1), k.delta(f[0], f[1]), "the good call after the refusals is still a delta")
    assert hosted(camera=C.byref(cam[2])) == 0
    same_text(text[:n.value], k.delta(f[1], f[2]), "and so is the host entry's")
    assert (text[n.value:] == 0xA5).all()


# ---- 3. the drop-in entries ----

@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_default_contexts_entry(ctx, kind):
    """keyframe, delta, a sphere moved between two calls, the other palette kind (a keyframe), trt_shutdown, keyframe"""
    half, k = is_half(kind), A.KINDS[kind]
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    cams = D.anim_cameras([0, 1, 2], W, H_)
    base = D.scene("demo")
    f0, f1 = frames_of("demo", [0, 1])
    f2 = D.oracle_rgb("demo", "synth", W, H_, 2, B, SPP, moved=True)
    term = k.terminal(W, H_)
    frame = lambda scene, h=half: hip.render_frame_ansi256_delta(scene, W, H_, B, SPP, half=h)
    try:
        got = frame(base.with_camera(cams[0]))
        same_text(got, k.keyframe(f0), "keyframe")
        term.feed(got).shows(f0, "keyframe")
        got = frame(base.with_camera(cams[1]))
        same_text(got, k.delta(f0, f1), "delta")
        term.feed(got).shows(f1, "delta")
        got = frame(D.moved_scene(base.with_camera(cams[2])))
        same_text(got, k.delta(f1, f2), "a sphere moved")
        term.feed(got).shows(f2, "a sphere moved")
        other = A.KINDS["full256" if half else "half256"]
        same_text(frame(base.with_camera(cams[1]), not half), other.keyframe(f1), "the other palette kind: its keyframe")
        same_text(hip.render_frame_ansi_delta(base.with_camera(cams[0]), W, H_, B, SPP), D.full_text(f0), "the 24-bit kind behind it: its keyframe")
        same_text(frame(base.with_camera(cams[1])), k.keyframe(f1), "and this kind behind that: a keyframe")
        hip._check(hip.lib().trt_shutdown())
        same_text(frame(base.with_camera(cams[1])), k.keyframe(f1), "keyframe after trt_shutdown")
        lib, scene, n = hip.lib(), base.as_scene(), C.c_size_t(0)
        entry = getattr(lib, "trt_render_frame_ansi256_delta" + ("_half" if half else ""))
        out = np.full(k.capacity(W, H_), 0xA5, dtype=np.uint8)
        assert entry(None, W, H_, B, SPP, out.ctypes.data, out.size, C.byref(n)) == ARGUMENT
        assert entry(C.byref(scene), W, H_, B, SPP, None, out.size, C.byref(n)) == ARGUMENT
        assert entry(C.byref(scene), W, H_, B, SPP, out.ctypes.data, out.size, None) == ARGUMENT
        assert entry(C.byref(scene), 100000, 1, B, SPP, out.ctypes.data, out.size, C.byref(n)) == ARGUMENT
        assert entry(C.byref(scene), W, H_, B, SPP, out.ctypes.data, out.size - 1, C.byref(n)) == CAPACITY
        assert (out == 0xA5).all()
    finally:
        hip._check(hip.lib().trt_shutdown())


# ---- 4. the demo ----

@pytest.mark.parametrize("flags", [["--delta256"], ["--delta256", "--half", "--batch=3"]], ids=["full", "half_batch3"])
def test_demo_program_draws_the_orbit_from_a_palette_keyframe_and_deltas(tmp_path, flags):
    """examples/trt_demo --delta256 at 67 x 13 for 3 frames: stdout is a keyframe of the palette text's length followed by texts the terminal
    model accepts, which leave it painted all over; stderr names the route; --256 --delta is still refused"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for face in T.FACES:
        (sky / (face + ".ppm")).write_bytes(T.golden_ppm_raw("colors", face))
    half, w, h = "--half" in flags, 67, 13
    n = hip.ansi256_bytes(w, h, half=half)
    run = subprocess.run([exe, str(sky), "3", str(w), str(h), "--step=0.0166667"] + flags, capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr[-500:]
    assert b"3 frames 67x13" in run.stderr and (b"as half-block 256-colour delta text" if half else b"as 256-colour delta text") in run.stderr
    assert b" fps, " in run.stderr and b"(%d each as whole texts)" % n in run.stderr
    assert n <= len(run.stdout) < 3 * n
    terminal = A.HalfTerminal if half else A.Terminal
    first = terminal(w, h).feed(run.stdout[:n])
    assert (first.grid >= 16).all(), "the first text is no keyframe"
    assert np.array_equal(first.grid if half else first.grid[:, ::2], A_read(run.stdout[:n], half))
    after = terminal(w, h).feed(run.stdout)
    assert (after.grid >= 16).all() and b"\033[0;0H" not in run.stdout[n:] and b"\n" not in run.stdout[n:]
    refused = subprocess.run([exe, str(sky), "1", str(w), str(h), "--256", "--delta"], capture_output=True, timeout=120)
    assert refused.returncode == 2 and not refused.stdout and b"--delta256" in refused.stderr
    for bad in (["--delta256", "--kitty"], ["--delta256", "--sixel"], ["--delta256", "--ansi"], ["--delta256", "--rgb8"], ["--256", "--delta256"]):
        refused = subprocess.run([exe, str(sky), "1", str(w), str(h)] + bad, capture_output=True, timeout=120)
        assert refused.returncode == 2 and not refused.stdout, bad


def A_read(text, half):
    """the entries a whole palette text shows, by the structural reader of the whole texts' tests"""
    import ansi256_support as P
    return P.read(text, half)
