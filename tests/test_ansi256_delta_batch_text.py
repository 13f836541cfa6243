"""The batch forms of the delta texts in the xterm 256-colour palette (trt_ansi256_delta[_half]_chain_from_rgb8_device,
trt_render_device_batch_ansi256_delta[_half], trt_render_host_batch_ansi256_delta[_half]; csrc/trt_ansi_delta_chain.h, trt_ansi_delta.hpp):
the texts of n frames back to back, placed by ONE prefix sum over the tiles of n pairs of frames.  The expected bytes never come from the
device route: they are the sequential host statement host.emitter_delta256_rgb8 of consecutive pattern frames or of consecutive
T.oracle_rgb8 frames, concatenated; keyframes are host.emitter_ansi256_rgb8's whole texts, and a model of a terminal must show every
frame's entries after its text.  Every device buffer stands between guard bytes of 0xA5, which also fill the unused room behind the last
text: none of them may change."""
import numpy as np
import pytest

import ansi256_delta_support as A
import ansi_delta_batch_support as S
import ansi_delta_support as D
from ansi_delta_support import B, SPP, W, frames_of, same_text
from ansi_delta_support import HEIGHT as H_
from terminalraytracer_amd import hip

pytestmark = pytest.mark.gpu
KIND_IDS = sorted(A.KINDS)
WIDTH, ROWS = 67, 13


@pytest.fixture(scope="module")
def ctx():
    yield from D.fresh_context()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield from D.restore_defaults(request)


def palette_chain(n, seed=0):
    """(shown, frames[n, 13, 67, 3]) whose steps a palette text tells apart: frame b from frame b - 1 by, in turn, 40 % of the pixels to
    other entries, the same entries in other bytes (a text of 0 bytes), every pixel to another entry than before and than its new left
    neighbour, the last pixel only"""
    rng = np.random.default_rng([seed, n])
    colours = A.entries()
    was = rng.integers(0, 240, (ROWS, WIDTH))
    shown = colours[was]
    frames = np.empty((n, ROWS, WIDTH, 3), dtype=np.uint8)
    last = shown
    for b in range(n):
        step = b % 4
        if step == 0:
            now = np.where(rng.random(was.shape) < 0.4, A._other_index(rng, was.shape, was), was)
            frames[b] = colours[now]
        elif step == 1:
            now, frames[b] = was, A.nudged(last) if (last == colours[was]).all() else colours[was]
        elif step == 2:
            now = was.copy()
            for c in range(WIDTH):
                now[:, c] = A._other_index(rng, (ROWS,), was[:, c], now[:, c - 1] if c else -1)
            frames[b] = colours[now]
        else:
            now = was.copy()
            now[-1, -1] = (was[-1, -1] + 1) % 240
            frames[b] = colours[now]
        was, last = now, frames[b]
    return np.ascontiguousarray(shown), frames


# ---- 1. the formatting alone ----

@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_formatting_alone_on_chains_of_frames(ctx, kind, n):
    """67 x 13, chains of any bytes from every starting step (ansi_delta_batch_support.chain) and a chain of palette entries: frames at odd
    addresses, the texts at the residues of their address modulo 4 in turn; lengths, bytes and guards are the host's; two frames of the same
    entries give a text of 0 bytes inside the chain; and the bytes are those of n calls of the one-pair entry"""
    k = A.KINDS[kind]
    for start in range(len(S.STEPS)):
        shown, frames = S.chain(WIDTH, ROWS, n, start)
        want = S.expected(k, shown, frames)
        S.same_texts(S.device_chain(ctx, k, shown, frames, start % 4, f"67x13 n={n} from {S.STEPS[start]}"), want, f"{kind} 67x13 n={n} from {S.STEPS[start]}")
        if S.STEPS[start] == "equal":
            assert want[0].size == 0
    shown, frames = palette_chain(n)
    want = S.expected(k, shown, frames)
    got = S.device_chain(ctx, k, shown, frames, 3, f"67x13 n={n}, palette entries")
    S.same_texts(got, want, f"{kind} 67x13 n={n}, palette entries")
    if n >= 2:
        assert want[1].size == 0 and (frames[1] != frames[0]).any(axis=2).all(), "other bytes of the same entries: a text of 0 bytes"
    if n >= 3 and kind == "half256":
        assert want[2].size == A.bound(WIDTH, ROWS, True) - 9 * (WIDTH - 1), "every cell changed: the bound, but for the odd frame's last text row"
    for b in range(n):
        last = shown if b == 0 else frames[b - 1]
        same_text(D.device_delta(ctx, k.single, k.capacity, np.array(last), np.array(frames[b]), 1, f"pair {b}"), got[b], f"{kind} n={n}: text {b} by the one-pair entry")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_terminal_fed_the_chain_shows_every_frame(ctx, kind):
    k = A.KINDS[kind]
    for shown, frames in (S.chain(WIDTH, ROWS, 8, 1), palette_chain(8)):
        term = k.terminal(WIDTH, ROWS).feed(k.keyframe(np.array(shown)))
        term.shows(shown, "the shown frame")
        for b, text in enumerate(S.device_chain(ctx, k, shown, frames, 2, "67x13")):
            term.feed(text).shows(frames[b], f"{kind} 67x13, text {b}")


@pytest.mark.parametrize("kind", KIND_IDS)
def test_the_formatting_entry_refuses_before_it_enqueues(ctx, kind):
    ARGUMENT, CAPACITY = -2, -4
    lib, k = hip.lib(), A.KINDS[kind]
    entry = getattr(lib, k.names[0])
    shown, frames = S.chain(7, 3, 8, 1)
    a, pa = D.at_odd_address(np.array(shown))
    f, pf = D.at_odd_address(np.array(frames))
    one = k.capacity(7, 3)
    room = S.Room(8 * one, 8)
    call = lambda c=ctx._h, s=pa, fr=pf, n=3, w=7, r=3, t=room.ptr, cap=3 * one, l=room.lengths_ptr: entry(c, s, fr, n, w, r, t, cap, l)
    too_wide, too_high = (100000, 199999) if kind == "half256" else (50000, 100000)
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


@pytest.mark.parametrize("kind", KIND_IDS)
def test_a_batch_a_single_call_and_a_batch_continue_one_another(ctx, kind):
    """a batch of 4 on a fresh shown frame: keyframe(f0) and three deltas; a single-frame call of camera 4: delta(f3, f4); a batch of cameras
    5..7: three deltas.  The terminal shows every frame; trt_batch_info tells what the 24-bit batch delta's tells; the batch's bytes are
    those of single calls on a second context"""
    k = A.KINDS[kind]
    ctx.set_scene(D.scene("demo"))
    rows = hip.RowSet.whole(W, H_)
    cams, f = D.anim_cameras(range(8), W, H_), frames_of("demo", range(8))
    term = k.terminal(W, H_)
    got = S.render_batch(ctx, k, cams[:4], rows, 1, "the first batch")
    S.same_texts(got, [k.keyframe(f[0])] + [k.delta(f[b - 1], f[b]) for b in (1, 2, 3)], f"{kind}, the first batch")
    fed(term, got, f[:4], "the first batch")
    info = ctx.batch_info()
    with hip.Context(0) as second:
        second.set_scene(D.scene("demo"))
        S.same_texts([k.render(second, cams[b], rows, offset=b % 4) for b in range(4)], got, f"{kind}: four single calls on a second context")
        twin = S.FULL if kind == "full256" else S.HALF
        S.render_batch(second, twin, cams[:4], rows, 0, "the 24-bit batch")
        assert second.batch_info() == info and info[0] == 4
    single = k.render(ctx, cams[4], rows, offset=2, what="a single-frame call behind the batch")
    same_text(single, k.delta(f[3], f[4]), "a single-frame call behind the batch")
    term.feed(single).shows(f[4], "a single-frame call behind the batch")
    got = S.render_batch(ctx, k, cams[5:8], rows, 3, "a batch behind the single-frame call")
    S.same_texts(got, [k.delta(f[b - 1], f[b]) for b in (5, 6, 7)], f"{kind}, a batch behind the single-frame call")
    fed(term, got, f[5:8], "a batch behind the single-frame call")
    assert ctx.batch_info()[0] == 3


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("kind", KIND_IDS)
def test_batches_of_every_length_from_a_keyframe_and_from_a_shown_frame(ctx, kind, n):
    """67 x 13: a batch of n on a fresh shown frame -- the keyframe and n - 1 deltas -- then a batch of n from the shown frame, its first
    camera the last one again: a text of 0 bytes in front of n - 1 deltas; the lengths are the texts'; the host entry returns the same bytes"""
    k = A.KINDS[kind]
    sc = D.scene("demo")
    ctx.set_scene(sc)
    rows = hip.RowSet.whole(WIDTH, ROWS)
    order = list(range(n)) + [n - 1] + list(range(n, 2 * n - 1))
    cams = D.anim_cameras(order, WIDTH, ROWS)
    f = [palette_frame(sc, cam) for cam in cams]
    first = S.render_batch(ctx, k, cams[:n], rows, 1, "from a keyframe")
    S.same_texts(first, [k.keyframe(f[0])] + [k.delta(f[b - 1], f[b]) for b in range(1, n)], f"{kind} n={n}, from a keyframe")
    second = S.render_batch(ctx, k, cams[n:], rows, 2, "from a shown frame")
    S.same_texts(second, [k.delta(f[b - 1], f[b]) for b in range(n, 2 * n)], f"{kind} n={n}, from a shown frame")
    assert second[0].size == 0, "the same camera again: the same entries"
    fed(k.terminal(WIDTH, ROWS), first + second, f, f"{kind} n={n}")
    ctx.ansi_delta_reset()
    hosted = k.render_host_batch(ctx, cams[:n], rows, B, SPP) + k.render_host_batch(ctx, cams[n:], rows, B, SPP)
    S.same_texts(hosted, first + second, f"{kind} n={n}, the host entry")


_FRAMES = {}


def palette_frame(sc, cam):
    """the oracle's frame of the camera at 67 x 13 as bytes, computed once"""
    import support as T
    key = cam.tobytes()
    if key not in _FRAMES:
        rgb = T.oracle_rgb8(T.oracle_render(sc.with_camera(cam), WIDTH, ROWS, B, SPP)[0])
        rgb.flags.writeable = False
        _FRAMES[key] = rgb
    return _FRAMES[key]
