"""The batch forms of the delta texts (trt_ansi_delta_chain_from_rgb8_device, trt_render_device_batch_ansi_delta, trt_render_host_batch_ansi_delta
and their _half forms; csrc/trt_ansi_delta_chain.h, trt_ansi_delta.hpp): the texts of n frames back to back, placed by ONE prefix sum over the
tiles of n pairs of frames -- three launches whatever n is.  The expected bytes never come from the device route: they are the sequential
host statements host.emitter_delta_rgb8 / host.emitter_delta_half_rgb8 of consecutive pattern frames or of consecutive T.oracle_rgb8 frames,
concatenated; keyframes are the host emitters' whole texts, and a model of a terminal must show every frame after its text.  Every device
buffer stands between guard bytes of 0xA5, which also fill the unused room behind the last text: none of them may change.  Section 3
holds the ONE path behind all of these entries to what only it can break: the context's two frame buffers as they flip and grow under
single-frame calls and batches, the single frame's render route behind a batch, the one-pair timing entries."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ansi_delta_batch_support as S
import ansi_delta_half_support as H
import ansi_delta_support as D
import support as T
from ansi_delta_support import B, SPP, W, frames_of, same_text
from ansi_delta_support import HEIGHT as H_
from terminalraytracer_amd import hip

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4
KIND_IDS = sorted(S.KINDS)


@pytest.fixture(scope="module")
def ctx():
    yield from D.fresh_context()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield from D.restore_defaults(request)


# ---- 1. the formatting alone ----

SIZES = [(1, 1), (1, 3), (2, 1), (63, 2), (64, 3), (65, 5), (160, 47)]  # 160 x 47: three tiles and a partial one a frame, an odd last row
LARGE = {"full": (2047, 65, 130), "half": (2047, 131, 132)}  # n = 8: 1040 and 1056 tiles in all, frames begin inside a turn of the 1024-sum scan


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_formatting_alone_on_chains_of_pattern_frames(ctx, kind, n):
    """one cell to several tiles a frame, odd and even frames, steps that cycle from every starting point through equal frames, everything
    changed, 40 %, the frame before last, the first and the last cell; frames at odd addresses, the text at every residue of its address
    modulo 4: lengths, bytes and guards are the host's"""
    k = S.KINDS[kind]
    for w, rows in SIZES:
        for start in range(len(S.STEPS)):
            shown, frames = S.chain(w, rows, n, start)
            want = S.expected(k, shown, frames)
            for offset in range(4):
                S.same_texts(S.device_chain(ctx, k, shown, frames, offset, f"{w}x{rows} n={n} from {S.STEPS[start]}"), want,
                             f"{kind} {w}x{rows} n={n} from {S.STEPS[start]} at offset {offset}")
            if S.STEPS[start] == "equal":
                assert want[0].size == 0
            if n == 3 and S.STEPS[start] == "last only":
                assert want[1].size == 0, "a text of 0 bytes in the middle of a chain"


@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_chain_of_one_is_the_one_pair_entry(ctx, kind):
    """n = 1: the text and the length trt_ansi_delta(_half)_from_rgb8_device is expected to write, which it writes"""
    k = S.KINDS[kind]
    for w, rows in SIZES:
        shown, frames = S.chain(w, rows, 1, 2)
        want = k.delta(shown, frames[0])
        S.same_texts(S.device_chain(ctx, k, shown, frames, 1, f"{w}x{rows}"), [want], f"{kind} {w}x{rows}, a chain of one")
        same_text(D.device_delta(ctx, k.single, k.capacity, np.array(shown), np.array(frames[0]), 1, f"{w}x{rows}"), want, f"{kind} {w}x{rows}, the one-pair entry")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_more_tiles_in_all_than_one_turn_of_the_offsets_scan(ctx, kind):
    w, rows, tiles = LARGE[kind]
    k = S.KINDS[kind]
    assert -(-w * ((rows + 1) // 2 if kind == "half" else rows) // 1024) == tiles and 8 * tiles > 1024 and 1024 % tiles
    shown, frames = S.large_chain(w, rows)
    want = S.expected(k, shown, frames)
    # frame 3 repeats frame 2; in frame 5 every cell changed and horizontal neighbours differ (but where two old colours differ by 0x010101): the
    # bound, but for the 17 bytes a cell that an odd frame's last text row saves on its black lower halves
    assert want[3].size == 0 and want[5].size > 0.99 * (H.bound if kind == "half" else D.bound)(w, rows)
    S.same_texts(S.device_chain(ctx, k, shown, frames, 3, f"{w}x{rows} n=8"), want, f"{kind} {w}x{rows} n=8")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_terminal_fed_the_chain_shows_every_frame(ctx, kind):
    """fed text by text behind the host's whole text of the shown frame, the terminal model shows frame after frame; in the odd-row sizes
    the next frame lies directly behind a frame's last pixel row, and the last text row's lower halves stay black in every half-block text"""
    k = S.KINDS[kind]
    for w, rows in [(1, 1), (1, 3), (2, 1), (64, 3), (65, 5), (160, 47)]:
        shown, frames = S.chain(w, rows, 8, 1)
        term = k.terminal(w, rows).feed(k.keyframe(np.array(shown)))
        term.shows(shown, "the shown frame")
        for b, text in enumerate(S.device_chain(ctx, k, shown, frames, 2, f"{w}x{rows}")):
            term.feed(text).shows(frames[b], f"{kind} {w}x{rows}, text {b}")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_formatting_entry_refuses_before_it_enqueues(ctx, kind):
    lib, k = hip.lib(), S.KINDS[kind]
    entry = getattr(lib, k.names[0])
    shown, frames = S.chain(7, 3, 8, 1)
    a, pa = D.at_odd_address(np.array(shown))
    f, pf = D.at_odd_address(np.array(frames))
    one = k.capacity(7, 3)
    room = S.Room(8 * one, 8)
    call = lambda c=ctx._h, s=pa, fr=pf, n=3, w=7, r=3, t=room.ptr, cap=3 * one, l=room.lengths_ptr: entry(c, s, fr, n, w, r, t, cap, l)
    too_wide, too_high = (100000, 199999) if kind == "half" else (50000, 100000)
    for bad in (dict(c=None), dict(s=None), dict(fr=None), dict(t=None), dict(l=None), dict(n=0), dict(n=9, cap=9 * one), dict(n=-1), dict(w=0), dict(r=0),
                dict(w=too_wide, cap=1 << 40), dict(r=too_high, cap=1 << 40)):
        assert call(**bad) == ARGUMENT, bad
    assert call(cap=3 * one - 1) == CAPACITY
    assert call(n=8, cap=8 * one - 1) == CAPACITY
    assert room.untouched(ctx)
    room3 = S.Room(3 * one, 3)
    assert call(t=room3.ptr, l=room3.lengths_ptr) == 0
    S.same_texts(room3.texts(ctx), S.expected(k, shown, frames[:3]), "the good call after the refusals")
    room3 = S.Room(3 * one, 3, 1)
    ms = k.chain_times(ctx, pa, pf, 3, 7, 3, room3.ptr, room3.capacity, room3.lengths_ptr)
    assert len(ms) == 3 and all(t >= 0 for t in ms)
    S.same_texts(room3.texts(ctx), S.expected(k, shown, frames[:3]), "the timing entry writes the same texts")


# ---- 2. the render entries ----

def fed(term, texts, frames, what):
    for b, text in enumerate(texts):
        term.feed(text).shows(frames[b], f"{what}, text {b}")


@pytest.mark.parametrize("scene_kind", ["demo", "synth64"])
@pytest.mark.parametrize("kernel", [hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER], ids=["production", "reference_order"])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_batch_a_single_call_and_a_batch_continue_one_another(ctx, kind, kernel, scene_kind):
    """a batch of 4 on a fresh shown frame: keyframe(f0), delta(f0, f1), delta(f1, f2), delta(f2, f3); a single-frame call of camera 4:
    delta(f3, f4); a batch of cameras 5..7: three deltas.  The terminal shows every frame.  Then the same batch over a shard's rows."""
    k = S.KINDS[kind]
    ctx.set_scene(D.scene(scene_kind))
    ctx.set_kernel(kernel)
    rows = hip.RowSet.whole(W, H_)
    cams, f = D.anim_cameras(range(8), W, H_), frames_of(scene_kind, range(8))
    term = k.terminal(W, H_)
    got = S.render_batch(ctx, k, cams[:4], rows, 1, "the first batch")
    S.same_texts(got, [k.keyframe(f[0])] + [k.delta(f[b - 1], f[b]) for b in (1, 2, 3)], f"{kind} {scene_kind}, the first batch")
    fed(term, got, f[:4], "the first batch")
    frames, launches = ctx.batch_info()
    assert frames == 4 and (launches == 4 if kernel == hip.Context.REFERENCE_ORDER else 1 <= launches <= 4)
    single = k.render(ctx, cams[4], rows, offset=2, what="a single-frame call behind the batch")
    same_text(single, k.delta(f[3], f[4]), "a single-frame call behind the batch")
    term.feed(single).shows(f[4], "a single-frame call behind the batch")
    got = S.render_batch(ctx, k, cams[5:8], rows, 3, "a batch behind the single-frame call")
    S.same_texts(got, [k.delta(f[b - 1], f[b]) for b in (5, 6, 7)], f"{kind} {scene_kind}, a batch behind the single-frame call")
    fed(term, got, f[5:8], "a batch behind the single-frame call")
    assert ctx.batch_info()[0] == 3
    # another rowset: a keyframe of the shard's rows, rows counted from its first one
    shard = hip.RowSet(W, H_, 8, 1, 3)
    fs = frames_of(scene_kind, range(4), shard)
    got = S.render_batch(ctx, k, cams[:4], shard, 2, "a shard")
    S.same_texts(got, [k.keyframe(fs[0])] + [k.delta(fs[b - 1], fs[b]) for b in (1, 2, 3)], f"{kind} {scene_kind}, a shard")
    fed(k.terminal(W, fs[0].shape[0]), got, fs, "a shard")


def test_an_odd_frame_in_half_block_cells(ctx):
    """160 x 47: the last text row's lower halves are black in every text of the batch, though frame b + 1 follows frame b directly"""
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, 47)
    cams, f = D.anim_cameras(range(4), W, 47), frames_of("demo", range(4), h=47)
    got = S.render_batch(ctx, S.HALF, cams, rows, 1, "160x47")
    S.same_texts(got, [S.HALF.keyframe(f[0])] + [S.HALF.delta(f[b - 1], f[b]) for b in (1, 2, 3)], "160x47")
    fed(H.Terminal(W, 47), got, f, "160x47")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_other_kind_a_reset_and_the_same_camera_twice(ctx, kind):
    k, other = S.KINDS[kind], S.KINDS["full" if kind == "half" else "half"]
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H_)
    cams, f = D.anim_cameras(range(6), W, H_), frames_of("demo", range(6))
    S.same_texts(S.render_batch(ctx, k, cams[:2], rows), [k.keyframe(f[0]), k.delta(f[0], f[1])], "a batch of two")
    S.same_texts(S.render_batch(ctx, other, cams[2:4], rows, 1), [other.keyframe(f[2]), other.delta(f[2], f[3])],
                 "a batch of the other kind: its first text is that kind's keyframe")
    same_text(k.render(ctx, cams[4], rows, offset=2), k.keyframe(f[4]), "a single-frame call of this kind behind it: a keyframe again")
    S.same_texts(S.render_batch(ctx, k, cams[[5, 5, 4]], rows, 3), [k.delta(f[4], f[5]), np.zeros(0, dtype=np.uint8), k.delta(f[5], f[4])],
                 "the same camera twice: a text of 0 bytes")
    ctx.ansi_delta_reset()
    S.same_texts(S.render_batch(ctx, k, cams[[4]], rows), [k.keyframe(f[4])], "after trt_ansi_delta_reset, a batch of one: the keyframe")
    S.same_texts(S.render_batch(ctx, k, cams[[4]], rows, 1), [np.zeros(0, dtype=np.uint8)], "a batch of one of the same camera")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_host_entries_return_the_device_entries_bytes(ctx, kind):
    k = S.KINDS[kind]
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H_)
    cams, f = D.anim_cameras(range(8), W, H_), frames_of("demo", range(8))
    got = k.render_host_batch(ctx, cams[:3], rows, B, SPP)
    assert isinstance(got, list) and all(t.dtype == np.uint8 for t in got)
    S.same_texts(got, [k.keyframe(f[0]), k.delta(f[0], f[1]), k.delta(f[1], f[2])], "host entry, a keyframe and two deltas")
    S.same_texts(S.render_batch(ctx, k, cams[3:5], rows, 1), [k.delta(f[2], f[3]), k.delta(f[3], f[4])], "device entry behind the host entry")
    S.same_texts(k.render_host_batch(ctx, cams[5:8], rows, B, SPP), [k.delta(f[b - 1], f[b]) for b in (5, 6, 7)], "host entry behind the device entry")
    assert ctx.batch_info()[0] == 3


@pytest.mark.parametrize("kind", KIND_IDS)
def test_refusals_keep_the_shown_frame(ctx, kind):
    lib, k = hip.lib(), S.KINDS[kind]
    device_entry, host_entry = getattr(lib, k.names[1]), getattr(lib, k.names[2])
    rows, bad_rows = hip.RowSet.whole(W, H_), hip.RowSet(0, H_, H_, 0, 1)
    cams = np.ascontiguousarray(D.anim_cameras(range(8), W, H_))
    nine = np.ascontiguousarray(np.concatenate([cams, cams[:1]]))
    other_screen = cams[:2].copy()
    other_screen[1, 13] *= 2
    f = frames_of("demo", range(4))
    one = k.capacity(W, H_)
    room = S.Room(9 * one, 8)
    text = np.full(9 * one, 0xA5, dtype=np.uint8)
    lengths = (C.c_size_t * 9)(*([77] * 9))
    with hip.Context(0) as empty:
        assert device_entry(empty._h, cams.ctypes.data, 2, C.byref(rows), B, SPP, room.ptr, 2 * one, room.lengths_ptr) == NO_SCENE
        assert host_entry(empty._h, cams.ctypes.data, 2, C.byref(rows), B, SPP, text.ctypes.data, 2 * one, lengths) == NO_SCENE
    ctx.set_scene(D.scene("demo"))
    S.same_texts(S.render_batch(ctx, k, cams[:2], rows), [k.keyframe(f[0]), k.delta(f[0], f[1])], "a keyframe and a delta")
    device = lambda c=ctx._h, cm=cams[2:].ctypes.data, n=2, rs=C.byref(rows), bl=B, out=room.ptr, cap=2 * one, l=room.lengths_ptr: \
        device_entry(c, cm, n, rs, bl, SPP, out, cap, l)
    hosted = lambda c=ctx._h, cm=cams[2:].ctypes.data, n=2, rs=C.byref(rows), bl=B, out=text.ctypes.data, cap=2 * one, l=lengths: \
        host_entry(c, cm, n, rs, bl, SPP, out, cap, l)
    for entry in (device, hosted):
        for bad in (dict(c=None), dict(cm=None), dict(rs=None), dict(out=None), dict(l=None), dict(rs=C.byref(bad_rows)), dict(bl=0), dict(n=0),
                    dict(n=9, cm=nine.ctypes.data, cap=9 * one), dict(cm=other_screen.ctypes.data)):
            assert entry(**bad) == ARGUMENT, bad
        assert entry(cap=2 * one - 1) == CAPACITY
        with hip.Context(0) as sharer:  # tables shared, either side: the eye slots a batch would build its tables in are the sharers'
            sharer.share_scene(ctx)
            assert entry() == CAPACITY and "shared" in lib.trt_last_error().decode()
    assert room.untouched(ctx), "a refused device entry wrote to the caller's buffer"
    assert (text == 0xA5).all() and list(lengths) == [77] * 9, "a refused host entry wrote to the caller's buffer"
    S.same_texts(S.render_batch(ctx, k, cams[2:3], rows, 1), [k.delta(f[1], f[2])], "the good call after the refusals is still a delta")
    assert hosted(cm=cams[3:].ctypes.data, n=1) == 0
    same_text(text[:lengths[0]], k.delta(f[2], f[3]), "and so is the host entry's")
    assert (text[lengths[0]:] == 0xA5).all() and list(lengths)[1:] == [77] * 8


# ---- 3. one path: the context's two frame buffers flip under single-frame calls and batches alike; the one-pair entries are chains of one ----

WHOLE, SHARD = hip.RowSet.whole(W, H_), hip.RowSet(W, H_, 8, 1, 3)
HOST_SINGLE = {"full": hip.Context.render_host_ansi_delta, "half": hip.Context.render_host_ansi_delta_half}
PAIR_TIMES = {"full": hip.Context.ansi_delta_kernel_times, "half": hip.Context.ansi_delta_half_kernel_times}
# (rowset, a batch entry?, the orbit's cameras): the shown frame is the last frame of a buffer of eight while the other buffer, of one frame,
# takes a batch of one, then lies in that buffer of one while the other takes eight; a shard's rows are a keyframe of another size
FLIPS = [(WHOLE, False, [0]), (WHOLE, True, [1, 2, 3, 4, 5, 6, 7, 0]), (WHOLE, True, [1]), (WHOLE, True, [2, 3, 4, 5, 6, 7, 0, 1]), (WHOLE, False, [2]),
         (SHARD, True, [0, 1]), (SHARD, False, [2])]
# a fresh context's buffers are of one frame each after two single-frame calls: the batch's buffer GROWS from one frame to eight while the
# shown frame lies in the other one, which a growing buffer's lost contents must not touch
GROWS = [(WHOLE, False, [0]), (WHOLE, False, [1]), (WHOLE, True, [2, 3, 4, 5, 6, 7, 0, 1]), (WHOLE, False, [2])]


def host_texts(ctx, kind, cams, rows, batch):
    """the texts of the kind's host entry, single-frame or batch, written into a buffer between guard bytes that the room behind the texts continues"""
    k = S.KINDS[kind]
    capacity = len(cams) * k.capacity(rows.width, D.owned_rows(rows))
    buf = np.full(D.GUARD + capacity + D.GUARD, 0xA5, dtype=np.uint8)
    out = buf[D.GUARD:D.GUARD + capacity]
    texts = k.render_host_batch(ctx, cams, rows, B, SPP, out) if batch else [HOST_SINGLE[kind](ctx, cams[0], rows, B, SPP, out)]
    texts = [t.copy() for t in texts]
    total = sum(t.size for t in texts)
    assert (buf[:D.GUARD] == 0xA5).all() and (buf[D.GUARD + total:] == 0xA5).all(), "bytes outside the texts were written"
    return texts


@pytest.mark.parametrize("steps", [FLIPS, GROWS], ids=["flips", "grows"])
@pytest.mark.parametrize("route", ["device", "host"])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_shown_frame_stays_where_it_was_rendered(kind, route, steps):
    """on a context of its own, whose buffers are as small as the calls so far made them: every text is the host's of the frame the terminal
    shows and the next one, and the terminal, fed text by text, shows every frame"""
    k = S.KINDS[kind]
    with hip.Context(0) as ctx:
        ctx.set_scene(D.scene("demo"))
        shown_rows = last = term = None
        for step, (rows, batch, indices) in enumerate(steps):
            what = f"{kind} {route} step {step}"
            cams, f = D.anim_cameras(indices, W, H_), frames_of("demo", indices, None if rows is WHOLE else rows)
            if route == "host":
                got = host_texts(ctx, kind, cams, rows, batch)
            elif batch:
                got = S.render_batch(ctx, k, cams, rows, step % 4, what)
            else:
                got = [k.render(ctx, cams[0], rows, offset=step % 4, what=what)]
            if rows is not shown_rows:
                shown_rows, term = rows, k.terminal(W, f[0].shape[0])
                first = k.keyframe(f[0])
            else:
                first = k.delta(last, f[0])
            S.same_texts(got, [first] + [k.delta(f[b - 1], f[b]) for b in range(1, len(f))], what)
            fed(term, got, f, what)
            last = f[-1]


@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_single_frame_call_is_not_a_batch(ctx, kind):
    """behind a batch of 3, a single-frame device call and a single-frame host call: trt_batch_info still tells of the batch, each is ONE
    launch, and the kernel that ran is the one trt_render_device_rgb8 runs for the rowset -- the single frame's form"""
    import torch
    k = S.KINDS[kind]
    ctx.set_scene(D.scene("demo"))
    ctx.set_kernel(hip.Context.PRODUCTION)
    cams, f = D.anim_cameras(range(5), W, H_), frames_of("demo", range(5))
    S.same_texts(S.render_batch(ctx, k, cams[:3], WHOLE), [k.keyframe(f[0]), k.delta(f[0], f[1]), k.delta(f[1], f[2])], "a batch of 3")
    info, launches = ctx.batch_info(), ctx.launch_count()
    assert info[0] == 3
    same_text(k.render(ctx, cams[3], WHOLE, offset=1), k.delta(f[2], f[3]), "a single-frame device call")
    assert ctx.batch_info() == info and ctx.launch_count() == launches + 1
    device_variant = ctx.render_variant()
    same_text(host_texts(ctx, kind, cams[4:5], WHOLE, False)[0], k.delta(f[3], f[4]), "a single-frame host call")
    assert ctx.batch_info() == info and ctx.launch_count() == launches + 2
    host_variant = ctx.render_variant()
    frame = torch.full((D.GUARD + f[4].size + D.GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device_rgb8(cams[4], WHOLE, B, SPP, frame.data_ptr() + D.GUARD, f[4].size)
    ctx.synchronize()
    assert device_variant == host_variant == ctx.render_variant()
    got = frame.cpu().numpy()
    assert (got[:D.GUARD] == 0xA5).all() and (got[-D.GUARD:] == 0xA5).all() and np.array_equal(got[D.GUARD:-D.GUARD], f[4].reshape(-1))


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_one_pair_timing_entry_writes_the_plain_entrys_text(ctx, kind):
    """trt_ansi_delta(_half)_kernel_times, a chain of one with events: three times, and the text and the length at an odd address"""
    k = S.KINDS[kind]
    for w, rows in [(W, H_), (W, 47)]:
        shown, frames = S.chain(w, rows, 1, 2)
        a, pa = D.at_odd_address(np.array(shown))
        b, pb = D.at_odd_address(np.array(frames[0]))
        room = D.Room(k.capacity(w, rows), 1)
        ms = PAIR_TIMES[kind](ctx, pa, pb, w, rows, room.ptr, room.capacity, room.length_ptr)
        assert len(ms) == 3 and all(t >= 0 for t in ms)
        timed = room.text(ctx, f"{kind} {w}x{rows}, the timing entry")
        same_text(timed, k.delta(shown, frames[0]), f"{kind} {w}x{rows}, the timing entry")
        same_text(timed, D.device_delta(ctx, k.single, k.capacity, np.array(shown), np.array(frames[0]), 1, f"{w}x{rows}"), f"{kind} {w}x{rows}, the plain entry")


# ---- 4. the demo ----

@pytest.mark.parametrize("frames", [4, 7])
@pytest.mark.parametrize("flags", [["--half", "--delta", "--batch=4"], ["--delta", "--batch=3"]], ids=["half_batch4", "full_batch3"])
def test_demo_program_renders_the_replay_ahead_in_batches(tmp_path, flags, frames):
    """examples/trt_demo --delta --batch=N over a whole number of batches and over a last batch that is shorter: stdout is byte for byte the
    unbatched --delta run's, and the terminal model is left with its picture"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for face in T.FACES:
        (sky / (face + ".ppm")).write_bytes(T.golden_ppm_raw("colors", face))
    common = [exe, str(sky), str(frames), str(W), str(H_), "--step=0.0166667"]
    batched = subprocess.run(common + flags, capture_output=True, timeout=120)
    assert batched.returncode == 0, batched.stderr[-500:]
    plain = subprocess.run(common + flags[:-1], capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr[-500:]
    assert f"{frames} frames 160x48".encode() in batched.stderr and b"delta text" in batched.stderr
    terminal = H.Terminal if "--half" in flags else D.Terminal
    want, got = terminal(W, H_).feed(plain.stdout), terminal(W, H_).feed(batched.stdout)
    assert (want.grid >= 0).all() and np.array_equal(got.grid, want.grid)
    assert batched.stdout == plain.stdout
