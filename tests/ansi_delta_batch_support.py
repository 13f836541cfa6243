"""What the tests of the batch forms of the delta texts add to ansi_delta_support and ansi_delta_half_support (test_ansi_delta_batch_text.py):
a room for n texts with n lengths, chains of pattern frames, the chain on the device at odd addresses, and what a kind of cell supplies to
the tests.  Expected bytes never come from a device route: they are the sequential emitters' texts of consecutive frames, concatenated."""
import collections
import functools

import numpy as np

import ansi_delta_half_support as H
import ansi_delta_support as D
from ansi_delta_support import GUARD, SENTINEL
from terminalraytracer_amd import hip, host

BATCH_MAX = 8


class Room:
    """`capacity` bytes of device memory `offset` bytes behind an 8-aligned address, filled with 0xA5 and with GUARD such bytes either side, and
    n uint64 on the device for the texts' lengths, a sentinel behind them"""

    def __init__(self, capacity, n, offset=0):
        import torch
        self.capacity, self.n, self.start = capacity, n, GUARD + offset
        self.buf = torch.full((GUARD + 8 + capacity + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.lengths = torch.full((max(n, 0) + 1,), SENTINEL, dtype=torch.int64, device="cuda:0")
        assert self.buf.data_ptr() % 8 == 0 and self.lengths.data_ptr() % 8 == 0
        torch.cuda.synchronize()  # the fills are on torch's stream, the kernels on the context's

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    @property
    def lengths_ptr(self):
        return self.lengths.data_ptr()

    def untouched(self, ctx):
        ctx.synchronize()
        return bool((self.lengths == SENTINEL).all().cpu()) and bool((self.buf == 0xA5).all().cpu())

    def texts(self, ctx, what=""):
        """the n texts, once every byte in front of them, behind the sum of their lengths -- the unused room -- and behind the room has been
        seen unchanged, and the uint64 behind the n lengths too"""
        ctx.synchronize()
        lengths = [int(k) for k in self.lengths.cpu()]
        assert lengths[self.n] == SENTINEL, f"{what}: more than {self.n} lengths were written"
        lengths = lengths[:self.n]
        total = sum(lengths)
        assert all(k >= 0 for k in lengths) and total <= self.capacity, f"{what}: lengths {lengths} in a room of {self.capacity}"
        got = self.buf.cpu().numpy()
        outside = np.concatenate([got[:self.start], got[self.start + total:]])
        assert (outside == 0xA5).all(), f"{what}: {int((outside != 0xA5).sum())} bytes outside the texts' {total} were written"
        ends = np.cumsum(lengths)
        return [got[self.start + end - k:self.start + end].copy() for k, end in zip(lengths, ends)]


def same_texts(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} texts for {len(want)}"
    for b, (g, w) in enumerate(zip(got, want)):
        D.same_text(g, w, f"{what}, text {b}")


# ---- chains of pattern frames ----

STEPS = ("equal", "all different", "forty", "back", "first only", "last only")


@functools.lru_cache(maxsize=None)
def chain(w, rows, n, start, seed=0):
    """(shown, frames[n, rows, w, 3]): frame b from frame b - 1 by step (start + b) % 6 -- equal frames (a text of 0 bytes), every cell changed
    with all neighbours different, 40 % changed, back to the frame before last, the first cell only, the last cell only"""
    rng = np.random.default_rng([seed, w, rows, n, start])
    shown = rng.integers(0, 256, (rows, w, 3), dtype=np.uint8)
    frames = np.empty((n, rows, w, 3), dtype=np.uint8)
    for b in range(n):
        last = shown if b == 0 else frames[b - 1]
        before_last = None if b == 0 else shown if b == 1 else frames[b - 2]
        step = STEPS[(start + b) % len(STEPS)]
        if step == "back" and before_last is None:
            step = "forty"
        nxt = last.copy()
        if step == "all different":
            for c in range(w):
                nxt[:, c] = D._other(rng, (rows,), last[:, c], nxt[:, c - 1] if c else last[:, c])
        elif step == "forty":
            change = rng.random((rows, w)) < 0.4
            nxt[change] = D._other(rng, (rows, w), last)[change]
        elif step == "back":
            nxt = before_last.copy()
        elif step == "first only":
            nxt[0, 0] = D._other(rng, (1,), last[0, 0][None])[0]
        elif step == "last only":
            nxt[-1, -1] = D._other(rng, (1,), last[-1, -1][None])[0]
        frames[b] = nxt
    shown.flags.writeable = frames.flags.writeable = False
    return shown, frames


def large_chain(w, rows, n=BATCH_MAX, seed=0):
    """more tiles than one turn of the scan: 40 % changed from frame to frame, one frame repeated, one with everything changed"""
    rng = np.random.default_rng([seed, w, rows])
    shown = rng.integers(0, 256, (rows, w, 3), dtype=np.uint8)
    frames = np.empty((n, rows, w, 3), dtype=np.uint8)
    for b in range(n):
        last = shown if b == 0 else frames[b - 1]
        if b == 3:
            frames[b] = last
        elif b == 5:
            frames[b] = last ^ np.uint8(0x80)
            frames[b][:, 1::2] ^= np.uint8(0x01)
        else:
            change = rng.random((rows, w)) < 0.4
            frames[b] = last
            frames[b][change] = rng.integers(0, 256, (int(change.sum()), 3), dtype=np.uint8)
    return shown, frames


def expected(kind, shown, frames):
    """the n texts of the chain, by the kind's sequential emitter"""
    return [kind.delta(shown if b == 0 else frames[b - 1], frames[b]) for b in range(len(frames))]


def device_chain(ctx, kind, shown, frames, offset=0, what=""):
    """the texts the kind's formatting entry writes for the chain: the shown frame and the n frames at odd addresses, the n frames back to
    back in an allocation that ends with the last one"""
    n, rows, w, _ = frames.shape
    a, pa = D.at_odd_address(np.array(shown))  # copies: the cached chains are read-only
    f, pf = D.at_odd_address(np.array(frames))
    room = Room(n * kind.capacity(w, rows), n, offset)
    kind.chain(ctx, pa, pf, n, w, rows, room.ptr, room.capacity, room.lengths_ptr)
    return room.texts(ctx, what)


def render_batch(ctx, kind, cams, rows, offset=0, what=""):
    """the texts the kind's render entry writes for the cameras"""
    room = Room(len(cams) * kind.capacity(rows.width, D.owned_rows(rows)), len(cams), offset)
    kind.render_batch(ctx, cams, rows, D.B, D.SPP, room.ptr, room.capacity, room.lengths_ptr)
    return room.texts(ctx, what)


# what a kind of cell supplies: ansi_delta_support's Kind (keyframe, delta, terminal, the single-frame render entry), and of the batch forms
# the capacity of one text, the formatting entry, the render entries, their names in the library, the one-pair formatting entry
Kind = collections.namedtuple("Kind", "keyframe delta terminal render capacity chain chain_times render_batch render_host_batch names single")
FULL = Kind(*D.FULL, hip.ansi_delta_capacity, hip.Context.ansi_delta_chain_from_rgb8, hip.Context.ansi_delta_chain_kernel_times,
            hip.Context.render_device_batch_ansi_delta, hip.Context.render_host_batch_ansi_delta,
            ("trt_ansi_delta_chain_from_rgb8_device", "trt_render_device_batch_ansi_delta", "trt_render_host_batch_ansi_delta"), hip.Context.ansi_delta_from_rgb8)
HALF = Kind(*H.HALF, hip.ansi_delta_half_capacity, hip.Context.ansi_delta_half_chain_from_rgb8, hip.Context.ansi_delta_half_chain_kernel_times,
            hip.Context.render_device_batch_ansi_delta_half, hip.Context.render_host_batch_ansi_delta_half,
            ("trt_ansi_delta_half_chain_from_rgb8_device", "trt_render_device_batch_ansi_delta_half", "trt_render_host_batch_ansi_delta_half"),
            hip.Context.ansi_delta_half_from_rgb8)
KINDS = {"full": FULL, "half": HALF}
