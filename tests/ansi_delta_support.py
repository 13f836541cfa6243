"""What the delta-text tests share (test_ansi_delta_host.py without a GPU, test_ansi_delta_text.py and test_ansi_delta_half_text.py with
one): a small model of a terminal, the families of frame pairs the format is exercised with, the oracle's frames of the demo orbit, and
the harness of the GPU tests of both kinds of cell -- guarded device buffers, frames at odd addresses with trap bytes behind them, the
keyframe-then-deltas sequence.  Expected texts never come from the library's device route: they are host.emitter_delta_rgb8 (the
sequential C statement) of T.oracle_rgb8 frames, and what the model shows is held against those frames themselves."""
import collections
import ctypes as C
import functools
import os
import re

import numpy as np

import support as T
from support import GUARD, anim_cameras, owned_rows  # noqa: F401 -- the delta tests take them from here
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S

DEFAULT = -2   # a cell painted after "\033[0m": the terminal's own background
NEVER = -1     # a cell nothing was painted on

_TOKEN = re.compile(rb"\x1b\[(\d*);(\d*)H|\x1b\[48;2;(\d+);(\d+);(\d+)m|(\x1b\[0m)|( +)|(\n)|(\x00+)")


class Terminal:
    """cursor, current background, a grid of column colours (a cell of the picture is two columns wide).  It understands exactly what the
    emitters write -- ESC[r;cH (a parameter 0 or empty counts as 1), ESC[48;2;r;g;bm, ESC[0m, space, newline, NUL -- and fails on anything else,
    on a space outside the screen and on a colour component above 255."""

    def __init__(self, width, rows):
        self.width, self.rows = width, rows
        self.grid = np.full((rows, 2 * width), NEVER, dtype=np.int64)
        self.row = self.col = 0
        self.background = DEFAULT

    def feed(self, text):
        data = bytes(np.asarray(text, dtype=np.uint8).tobytes()) if not isinstance(text, (bytes, bytearray)) else bytes(text)
        at = 0
        while at < len(data):
            m = _TOKEN.match(data, at)
            assert m, f"byte {at} of {len(data)}: the terminal model does not know {data[at:at + 12]!r}"
            if m.group(1) is not None:
                self.row, self.col = max(int(m.group(1) or 1), 1) - 1, max(int(m.group(2) or 1), 1) - 1
            elif m.group(3) is not None:
                r, g, b = int(m.group(3)), int(m.group(4)), int(m.group(5))
                assert max(r, g, b) <= 255, (at, r, g, b)
                self.background = r | g << 8 | b << 16
            elif m.group(6) is not None:
                self.background = DEFAULT
            elif m.group(7) is not None:
                n = len(m.group(7))
                assert self.row < self.rows and self.col + n <= 2 * self.width, f"byte {at}: {n} space(s) at row {self.row}, column {self.col} of a {self.rows} x {2 * self.width} screen"
                self.grid[self.row, self.col:self.col + n] = self.background
                self.col += n
            elif m.group(8) is not None:
                self.row, self.col = self.row + 1, 0
            at = m.end()
        return self

    def shows(self, rgb, what=""):
        """every cell shows its colour of the frame rgb [rows, width, 3], in both of its columns"""
        want = rgb[..., 0].astype(np.int64) | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2].astype(np.int64) << 16
        for half in (0, 1):
            got = self.grid[:, half::2]
            wrong = got != want
            if wrong.any():
                r, c = np.argwhere(wrong)[0]
                kind = {DEFAULT: "the default background", NEVER: "nothing"}.get(int(got[r, c]), f"{int(got[r, c]):06x}")
                raise AssertionError(f"{what}: {int(wrong.sum())} cells show another colour in column {half}; cell ({r}, {c}) shows {kind} for {int(want[r, c]):06x}")


def full_text(rgb):
    """the host emitter's buffer for a frame of bytes [rows, w, 3]"""
    rows, w, _ = rgb.shape
    e = host.Emitter(w, rows)
    try:
        e.patch_rgb8(rgb)
        return np.frombuffer(e.bytes(), dtype=np.uint8).copy()
    finally:
        e.close()


def bound(w, rows):
    return rows * (21 * w + 18)


# ---- frame pairs ----

FAMILIES = ("nothing", "all different", "all one colour", "alternate", "first only", "last only", "across rows", "left colour",
            "two colours 0.01", "two colours 0.4", "two colours 0.99", "full palette 0.01", "full palette 0.4", "full palette 0.99")


def _other(rng, shape, *avoid):
    """random colours [..., 3] that differ, cell by cell, from each of `avoid`"""
    out = rng.integers(0, 256, tuple(shape) + (3,), dtype=np.uint8)
    for _ in range(64):
        clash = np.zeros(shape, dtype=bool)
        for a in avoid:
            clash |= (out == a).all(axis=-1)
        if not clash.any():
            return out
        out[clash] = rng.integers(0, 256, (int(clash.sum()), 3), dtype=np.uint8)
    raise AssertionError("no colours found")


def pair(family, w, rows, seed=0):
    """(shown, next): two frames of bytes [rows, w, 3] of the family"""
    rng = np.random.default_rng([seed, FAMILIES.index(family), w, rows])
    shown = rng.integers(0, 256, (rows, w, 3), dtype=np.uint8)
    nxt = shown.copy()
    if family == "all different":  # column by column: different from the shown colour and from the new colour to the left
        for c in range(w):
            nxt[:, c] = _other(rng, (rows,), shown[:, c], nxt[:, c - 1] if c else shown[:, c])
    elif family == "all one colour":
        shown[...] = (0x10, 0x20, 0x30)
        shown[:, ::2, 0] = 0x11
        nxt[...] = (0xa0, 0xb0, 0xc0)
    elif family == "alternate":
        nxt[:, ::2] = _other(rng, nxt[:, ::2].shape[:2], shown[:, ::2])
    elif family == "first only":
        nxt[0, 0] = _other(rng, (1,), shown[0, 0][None])[0]
    elif family == "last only":
        nxt[-1, -1] = _other(rng, (1,), shown[-1, -1][None])[0]
    elif family == "across rows":  # into every row's last cell and out of the next row's first, one colour
        for r in range(max(rows - 1, 1)):
            shown[r, -2:], nxt[r, -2:] = (1, 1, 1), (0x7f, 0xff, 0)
            if r + 1 < rows:
                shown[r + 1, :2], nxt[r + 1, :2] = (2, 2, 2), (0x7f, 0xff, 0)
    elif family == "left colour":  # every third cell takes the colour of its unchanged left neighbour
        flat_shown, flat = shown.reshape(-1, 3), nxt.reshape(-1, 3)
        for p in range(1, flat.shape[0], 3):
            if (p % w) and (flat_shown[p] != flat_shown[p - 1]).any():
                flat[p] = flat[p - 1]
    elif family.startswith(("two colours", "full palette")):
        p = float(family.split()[-1])
        change = rng.random((rows, w)) < p
        if family.startswith("two"):
            shown = np.where(rng.random((rows, w, 1)) < 0.5, np.uint8(255), np.uint8(0)).repeat(3, axis=2).astype(np.uint8)
            nxt = shown.copy()
            nxt[change] ^= 255
        else:
            nxt[change] = _other(rng, (rows, w), shown)[change]
    else:
        assert family == "nothing", family
    return np.ascontiguousarray(shown), np.ascontiguousarray(nxt)


# ---- the oracle's orbit ----

@functools.lru_cache(maxsize=None)
def scene(kind, sky="synth"):
    cam = anim_cameras([0], 160, 48)[0]
    if kind == "demo":
        return S.demo_scene(T.sky(sky), cam)
    return S.synth_scene(64, T.sky(sky), cam, seed=11)


@functools.lru_cache(maxsize=None)
def oracle_rgb(kind, sky, w, h, index, b, spp, moved=False):
    """the oracle's frame `index` of the orbit as bytes [h, w, 3], computed once, never written to"""
    sc = scene(kind, sky).with_camera(anim_cameras([index], w, h)[0])
    if moved:
        sc = moved_scene(sc)
    rgb = T.oracle_rgb8(T.oracle_render(sc, w, h, b, spp)[0])
    rgb.flags.writeable = False
    return rgb


def moved_scene(sc):
    """the scene with its first sphere half a unit higher"""
    spheres = sc.spheres.copy()
    spheres[0, 1] += 0.5
    return sc.with_spheres(spheres)


# ---- the GPU tests' harness, for both kinds of cell ----

SENTINEL = 0x5A5A5A5A5A5A5A5A
W, HEIGHT, B, SPP = 160, 48, 4, 10


def fresh_context():
    """the body of a test module's `ctx` fixture"""
    c = hip.Context(0)
    yield c
    c.close()


def restore_defaults(request):
    """the body of a test module's autouse fixture: after a test that used `ctx`, the production kernel and no shown frame"""
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.set_kernel(hip.Context.PRODUCTION)
        c.ansi_delta_reset()


class Room:
    """`capacity` bytes of device memory `offset` bytes behind an 8-aligned address, filled with 0xA5 and with GUARD such bytes either side, and a
    uint64 on the device for the text's length"""

    def __init__(self, capacity, offset=0):
        import torch
        self.capacity, self.start = capacity, GUARD + offset
        self.buf = torch.full((GUARD + 8 + capacity + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.length = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda:0")
        assert self.buf.data_ptr() % 8 == 0 and self.length.data_ptr() % 8 == 0
        torch.cuda.synchronize()  # the fills are on torch's stream, the kernels on the context's

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    @property
    def length_ptr(self):
        return self.length.data_ptr()

    def untouched(self, ctx):
        ctx.synchronize()
        return int(self.length.cpu()[0]) == SENTINEL and bool((self.buf == 0xA5).all().cpu())

    def text(self, ctx, what=""):
        """the text, once every byte in front of it, behind its length and behind its room has been seen unchanged"""
        ctx.synchronize()
        n = int(self.length.cpu()[0])
        assert 0 <= n <= self.capacity, f"{what}: a length of {n} in a room of {self.capacity}"
        got = self.buf.cpu().numpy()
        outside = np.concatenate([got[:self.start], got[self.start + n:]])
        assert (outside == 0xA5).all(), f"{what}: {int((outside != 0xA5).sum())} bytes outside the text's {n} were written"
        return got[self.start:self.start + n].copy()


same_text = functools.partial(T.same_text, whose="the host's")


def at_odd_address(frame, behind=None):
    """the frame's bytes on the device, one byte behind an aligned address, followed directly by the bytes `behind` where given: (the
    tensor that owns them, the frame's address)"""
    import torch
    tail = 0 if behind is None else behind.size
    t = torch.zeros(frame.size + 1 + tail, dtype=torch.uint8, device="cuda:0")
    t[1:1 + frame.size] = torch.from_numpy(np.ascontiguousarray(frame).reshape(-1)).to("cuda:0")
    if tail:
        t[1 + frame.size:] = torch.from_numpy(behind).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr() + 1


def device_delta(ctx, from_rgb8, capacity, shown, nxt, offset=0, what="", trap=False):
    """the text the formatting entry `from_rgb8` (a method of hip.Context) writes for the pair, both frames at odd addresses.  trap: a further
    pixel row behind each frame, 0x00 behind `shown` and 0xFF behind `next` -- changed cells to a kernel that loaded it"""
    rows, w, _ = shown.shape
    a, pa = at_odd_address(shown, np.full(w * 3, 0x00, dtype=np.uint8) if trap else None)
    b, pb = at_odd_address(nxt, np.full(w * 3, 0xFF, dtype=np.uint8) if trap else None)
    room = Room(capacity(w, rows), offset)
    from_rgb8(ctx, pa, pb, w, rows, room.ptr, room.capacity, room.length_ptr)
    return room.text(ctx, what)


def frames_of(scene_kind, indices, rows=None, b=B, h=HEIGHT):
    out = [oracle_rgb(scene_kind, "synth", W, h, k, b, SPP) for k in indices]
    if rows is not None:
        owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(owned_rows(rows))]
        out = [np.ascontiguousarray(f[owned]) for f in out]
    return out


def render_text(ctx, render, capacity, cam, rows, offset=0, what=""):
    """the text the render entry `render` (a method of hip.Context) writes for the camera"""
    room = Room(capacity(rows.width, owned_rows(rows)), offset)
    render(ctx, cam, rows, B, SPP, room.ptr, room.capacity, room.length_ptr)
    return room.text(ctx, what)


def render_full(ctx, cam, rows, offset=0, what=""):
    return render_text(ctx, hip.Context.render_device_ansi_delta, hip.ansi_delta_capacity, cam, rows, offset, what)


# what a kind of cell supplies to check_sequence: the keyframe's text of a frame, the delta emitter of two, the terminal model, the render entry
Kind = collections.namedtuple("Kind", "keyframe delta terminal render")
FULL = Kind(full_text, host.emitter_delta_rgb8, Terminal, render_full)


def check_sequence(kind, ctx, scene_kind, rows, indices=(0, 1, 2, 3), between=None, what="", h=HEIGHT):
    """a keyframe, then deltas, of the Kind `kind` of cell over the scene `scene_kind`: the texts are the host's of the oracle's frames, and
    the terminal shows every frame"""
    cams = anim_cameras(indices, W, h)
    frames = frames_of(scene_kind, indices, rows, h=h)
    term = kind.terminal(W, frames[0].shape[0])
    for k in range(len(indices)):
        got = kind.render(ctx, cams[k], rows, offset=k % 4, what=f"{what} call {k}")
        want = kind.keyframe(frames[0]) if k == 0 else kind.delta(frames[k - 1], frames[k])
        same_text(got, want, f"{what} call {k}")
        term.feed(got).shows(frames[k], f"{what} call {k}")
        if between:
            between(k)
