"""What tests/test_stream_order.py is made of: the table of scenarios (read by the GPU tests and by the coverage check, which needs no
GPU), the gate -- a bounded delay in front of a scenario, so that everything the scenario enqueues stays queued until the host has issued
all of it --, guarded output slots with a snapshot taken on the stream, the raw calls with host memory the test owns and overwrites as soon
as a call returns, and the expected bytes.  Expected bytes never come from the device: they are T.oracle_render / T.oracle_rgb8 frames, the
host emitters' whole texts of them and the sequential delta emitters' texts, with a small model of which frame a context shows."""
import collections
import ctypes as C
import functools
import os
import re
import time

import numpy as np

import ansi_delta_half_support as H
import ansi_delta_support as D
import support as T
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import layout as L
from terminalraytracer_amd import scenes as S

W, HEIGHT, SPP = 67, 13, 3        # 2613 values a frame: odd, with a head and a tail at every byte alignment
CAMERAS = (0, 3, 6, 9)            # of the stored orbit (tests/golden/cameras_anim.npz)
BATCH = 3
GUARD, SENTINEL = D.GUARD, D.SENTINEL
FILL, SCRIBBLE, STALE = 0xA5, 0x3C, 0x11
CAPACITY = -4
GATE_FACTOR, GATE_MIN_MS, GATE_MAX_MS = 20.0, 50.0, 500.0

# ---- the table of scenarios ----

# (kind of output, batch form) of every render entry
KIND_OF = {"trt_render_device": ("doubles", False), "trt_render_device_rgb8": ("rgb8", False), "trt_render_device_ansi": ("ansi", False),
           "trt_render_device_ansi_half": ("ansi_half", False), "trt_render_device_ansi_delta": ("delta", False),
           "trt_render_device_ansi_delta_half": ("delta_half", False), "trt_render_device_batch": ("doubles", True),
           "trt_render_device_batch_rgb8": ("rgb8", True), "trt_render_device_batch_ansi": ("ansi", True),
           "trt_render_device_batch_ansi_half": ("ansi_half", True), "trt_render_device_batch_ansi_delta": ("delta", True),
           "trt_render_device_batch_ansi_delta_half": ("delta_half", True)}

# one call of a render entry: the context that makes it (an index into the scenario's contexts), the cameras (indices into CAMERAS; one unless the
# entry is a batch form), and whether trt_ansi_delta_reset goes in front of it
Step = collections.namedtuple("Step", "entry cams who reset", defaults=(0, False))
# one call of a formatting entry: n frames (1 unless the entry is a chain)
Format = collections.namedtuple("Format", "entry n")

FORMATTING = (Format("trt_quantize_device", 1), Format("trt_ansi_from_rgb8_device", 1), Format("trt_ansi_half_from_rgb8_device", 1),
              Format("trt_ansi_delta_from_rgb8_device", 1), Format("trt_ansi_delta_half_from_rgb8_device", 1),
              Format("trt_ansi_delta_chain_from_rgb8_device", BATCH), Format("trt_ansi_delta_half_chain_from_rgb8_device", BATCH))

RUN = (Step("trt_render_device", (0,)), Step("trt_render_device_rgb8", (1,)), Step("trt_render_device_ansi", (2,)),
       Step("trt_render_device_ansi_half", (3,)),
       Step("trt_render_device_ansi_delta", (0,)),       # a keyframe
       Step("trt_render_device_ansi_delta", (1,)), Step("trt_render_device_ansi_delta", (2,)),
       Step("trt_render_device_ansi_delta_half", (3,)),  # a keyframe: the kind changed
       Step("trt_render_device_ansi_delta_half", (0,)),
       Step("trt_render_device_batch", (1, 2, 3)), Step("trt_render_device_batch_rgb8", (2, 3, 0)), Step("trt_render_device_batch_ansi", (3, 0, 1)),
       Step("trt_render_device_batch_ansi_half", (0, 1, 2)),
       Step("trt_render_device_ansi_delta", (3,)),                  # a keyframe again, for the batch to continue from
       Step("trt_render_device_batch_ansi_delta", (0, 1, 2)),       # continues a single frame's delta
       Step("trt_render_device_batch_ansi_delta_half", (3, 0, 1)),  # a keyframe and a chain of two behind it
       Step("trt_render_device_ansi_delta", (2,), 0, True),         # a keyframe: the reset
       Step("trt_render_device", (0,)))
FIRST_HALF = RUN[:9]

# two contexts that share one scene's tables, each in its own eye slot and on its own stream, taking turns
SHARED = (Step("trt_render_device", (0,), 0), Step("trt_render_device_rgb8", (1,), 1), Step("trt_render_device_ansi", (2,), 0),
          Step("trt_render_device_ansi_half", (3,), 1), Step("trt_render_device_ansi_delta", (1,), 0), Step("trt_render_device_ansi_delta_half", (2,), 1),
          Step("trt_render_device_ansi_delta", (3,), 0), Step("trt_render_device_ansi_delta_half", (0,), 1), Step("trt_render_device", (2,), 1),
          Step("trt_render_device_rgb8", (3,), 0))

# the frames of the scenario whose other calls may have to wait (test_stream_order.py states the calls between them)
WAITING = (Step("trt_render_device", (0,)), Step("trt_render_device_rgb8", (1,)), Step("trt_render_device_batch_rgb8", (1, 2, 3)),
           Step("trt_render_device_ansi_delta", (2,)), Step("trt_render_device_batch_ansi_delta", (1, 2, 3)))

SCENARIOS = {"formatting alone": FORMATTING, "a run of frames": RUN, "the context's own stream": FIRST_HALF, "two contexts, one scene": SHARED,
             "calls that may have to wait": WAITING}

# Entries that wait for the device in the steady state (every buffer grown, every table built), with the reason, which include/trt_hip.h states
# in the entry's comment.  None does: every guard synchronisation of the library is on a path that grows a buffer or rewrites a table.
WAITS = {}


def asynchronous_entries(header=os.path.join(T.ROOT, "include", "trt_hip.h")):
    """every entry include/trt_hip.h declares asynchronous on the context's stream: trt_render_device*, *_from_rgb8_device, trt_quantize_device"""
    with open(header) as fh:
        names = re.findall(r"^int\s+(trt_\w+)\s*\(", fh.read(), re.M)
    return sorted(n for n in names if n.startswith("trt_render_device") or n.endswith("_from_rgb8_device") or n == "trt_quantize_device")


def covered_entries():
    return {step.entry for steps in SCENARIOS.values() for step in steps}


# ---- scenes, routes and the oracle's frames ----

def cameras(w=W, h=HEIGHT, screen=None):
    """the four cameras for a w x h frame; screen = d: a screen of w / d by h / d, so that a pixel measures 1 / d whatever the size"""
    cams = D.anim_cameras(CAMERAS, w, h)
    if screen:
        cams[:, 13], cams[:, 14] = w / float(screen), h / float(screen)
    return cams


@functools.lru_cache(maxsize=None)
def scene(name):
    cam = cameras()[0]
    if name == "demo":
        return S.demo_scene(T.sky("synth"), cam)
    assert name == "synth24"
    return S.synth_scene_lights(24, 3, T.sky("synth"), cam, seed=11)  # three directional lights and the point light


# route: (scene, bounce limit, set-up of the context)
Route = collections.namedtuple("Route", "scene bounce kernel compaction image")
ROUTES = {"plain rounds": Route("demo", 3, hip.Context.PRODUCTION, -1, -1),
          "decoupled rounds": Route("synth24", 4, hip.Context.PRODUCTION, 1, -1),
          "scene image in device memory": Route("synth24", 2, hip.Context.PRODUCTION, 1, 1),
          "reference-order kernel": Route("synth24", 2, hip.Context.REFERENCE_ORDER, -1, -1)}


def configure(ctx, route):
    ctx.set_kernel(route.kernel)
    ctx.set_compaction(route.compaction)
    ctx.set_scene_image(route.image)
    ctx.set_scene(scene(route.scene))


@functools.lru_cache(maxsize=None)
def oracle_px(scene_name, cam, bounce, spp=SPP, w=W, h=HEIGHT, ior=None, screen=None):
    """the oracle's frame of camera CAMERAS[cam], doubles [h, w, 3], computed once and never written to"""
    sc = scene(scene_name).with_camera(cameras(w, h, screen)[cam])
    px = T.oracle_render(sc, w, h, bounce, spp)[0] if ior is None else T.oracle_render_refractive(sc, np.array(ior), w, h, bounce, spp)[0]
    px.flags.writeable = False
    return px


@functools.lru_cache(maxsize=None)
def oracle_rgb(scene_name, cam, bounce, spp=SPP, w=W, h=HEIGHT, ior=None, screen=None):
    rgb = T.oracle_rgb8(oracle_px(scene_name, cam, bounce, spp, w, h, ior, screen))
    rgb.flags.writeable = False
    return rgb


class Frames:
    """the oracle's frames of one state of a context: scene, bounce limit, rays per pixel, size, refraction indices, the cameras' screen"""

    def __init__(self, scene_name, bounce, spp=SPP, w=W, h=HEIGHT, ior=None, screen=None):
        self.key = (scene_name, bounce, spp, w, h, None if ior is None else tuple(float(x) for x in ior), screen)
        self.bounce, self.spp, self.w, self.h, self.screen = bounce, spp, w, h, screen

    def camera(self, cam):
        return cameras(self.w, self.h, self.screen)[cam]

    def px(self, cam):
        return oracle_px(self.key[0], cam, *self.key[1:])

    def rgb(self, cam):
        return oracle_rgb(self.key[0], cam, *self.key[1:])


# ---- expected bytes ----

WHOLE = {"ansi": D.full_text, "ansi_half": host.emitter_half_rgb8, "delta": D.full_text, "delta_half": host.emitter_half_rgb8}
DELTA = {"delta": host.emitter_delta_rgb8, "delta_half": host.emitter_delta_half_rgb8}
TERMINAL = {"delta": D.Terminal, "delta_half": H.Terminal}


def capacity_of(kind, w, rows, n):
    one = {"doubles": w * rows * 24, "rgb8": w * rows * 3, "ansi": hip.ansi_bytes(w, rows), "ansi_half": hip.ansi_half_bytes(w, rows),
           "delta": hip.ansi_delta_capacity(w, rows), "delta_half": hip.ansi_delta_half_capacity(w, rows)}[kind]
    return n * one


class Shown:
    """which frame a context shows, and as which kind of text (trt_render_device_ansi_delta's rules)"""

    def __init__(self):
        self.kind = self.frame = self.terminal = None

    def reset(self):
        self.kind = self.frame = None


Want = collections.namedtuple("Want", "data lengths texts")  # texts: [(text, frame, keyframe)] of a delta entry, for the terminal's model


def expected(kind, frames, cams, shown):
    """what a call of the kind writes for the cameras: the bytes back to back, the lengths of a delta entry's texts; `shown` moves on"""
    if kind == "doubles":
        return Want(np.concatenate([np.ascontiguousarray(frames.px(c)).view(np.uint8).reshape(-1) for c in cams]), None, None)
    if kind == "rgb8":
        return Want(np.concatenate([frames.rgb(c).reshape(-1) for c in cams]), None, None)
    if kind in ("ansi", "ansi_half"):
        return Want(np.concatenate([WHOLE[kind](frames.rgb(c)) for c in cams]), None, None)
    texts = []
    for c in cams:
        rgb = frames.rgb(c)
        key = shown.kind != kind or shown.frame is None or shown.frame.shape != rgb.shape
        texts.append((WHOLE[kind](rgb) if key else DELTA[kind](shown.frame, rgb), rgb, key))
        shown.kind, shown.frame = kind, rgb
    return Want(np.concatenate([t for t, _, _ in texts]), [int(t.size) for t, _, _ in texts], texts)


# ---- the gate ----

class Gate:
    """A bounded delay on a stream: torch.cuda._sleep of a number of clock ticks calibrated once with HIP events (a chain of large elementwise
    operations where _sleep's clock is of no use).  Never a kernel that waits for the host.  `end` is recorded behind the delay: end.query()
    is what the host knows of whether the gate is still closed."""
    ticks_per_ms = None
    chain = None  # (tensor, ms per operation): the stand-in

    @classmethod
    def calibrate(cls):
        import torch
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ticks = 2_000_000
        a.record()
        torch.cuda._sleep(ticks)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if 0.2 <= ms <= 200.0:
            cls.ticks_per_ms = ticks / ms
            return
        x = torch.ones(1 << 25, dtype=torch.float32, device="cuda:0")
        x.mul_(1.0)
        torch.cuda.synchronize()
        a.record()
        for _ in range(32):
            x.mul_(1.0)
        b.record()
        torch.cuda.synchronize()
        cls.chain = (x, a.elapsed_time(b) / 32)

    def __init__(self, stream, ms):
        import torch
        if Gate.ticks_per_ms is None and Gate.chain is None:
            Gate.calibrate()
        self.asked_ms = ms
        self.start, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.start.record()
            if Gate.ticks_per_ms is not None:
                torch.cuda._sleep(int(ms * Gate.ticks_per_ms))
            else:
                x, each = Gate.chain
                for _ in range(int(ms / each) + 1):
                    x.mul_(1.0)
            self.end.record()

    def closed(self):
        return not self.end.query()

    def achieved_ms(self):
        """after the stream has been synchronised"""
        return self.start.elapsed_time(self.end)


def gate_ms(warm_up_seconds):
    return min(max(GATE_FACTOR * warm_up_seconds * 1e3, GATE_MIN_MS), GATE_MAX_MS)


REPORT = []


def report(name, warm_up_seconds, gate, closed):
    line = (f"stream order: {name}: E = {warm_up_seconds * 1e3:.3f} ms, gate asked {gate.asked_ms:.1f} ms, achieved {gate.achieved_ms():.1f} ms, "
            f"still closed after the last call: {closed}")
    REPORT.append(line)
    print(line)


# ---- device memory of one call ----

class Slot:
    """A call's output: `capacity` bytes `offset` bytes behind an aligned address with GUARD bytes either side, n + 1 uint64 for a delta entry's
    lengths, and a snapshot of both.  Until arm() the output holds other bytes; arm() fills output and guards with 0xA5 and take() copies them
    to the snapshot and scribbles over the output at once -- all of it on the current stream."""

    def __init__(self, capacity, n=0, offset=0):
        import torch
        self.capacity, self.n, self.start = capacity, n, GUARD + offset
        size = GUARD + 8 + capacity + GUARD
        self.out = torch.full((size,), STALE, dtype=torch.uint8, device="cuda:0")
        self.snap = torch.zeros(size, dtype=torch.uint8, device="cuda:0")
        self.lengths = torch.full((n + 1,), 0x1111, dtype=torch.int64, device="cuda:0")
        self.snap_lengths = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        assert self.out.data_ptr() % 8 == 0 and self.lengths.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return self.out.data_ptr() + self.start

    @property
    def lengths_ptr(self):
        return self.lengths.data_ptr()

    def arm(self):
        self.out.fill_(FILL)
        self.lengths.fill_(SENTINEL)

    def take(self):
        self.snap.copy_(self.out)
        self.snap_lengths.copy_(self.lengths)
        self.out.fill_(SCRIBBLE)
        self.lengths.fill_(-1)

    def untouched(self):
        """after the synchronisation: nothing was written between arm() and take()"""
        return bool((self.snap == FILL).all().cpu()) and bool((self.snap_lengths == SENTINEL).all().cpu())

    def check(self, want, what):
        """after the synchronisation: the snapshot holds the expected bytes, the lengths are the emitter's, every guard byte is intact"""
        got = self.snap.cpu().numpy()
        size = int(want.data.size)
        assert size <= self.capacity, f"{what}: {size} expected bytes in a room of {self.capacity}"
        if want.lengths is not None:
            lengths = [int(k) for k in self.snap_lengths.cpu()]
            assert lengths[self.n] == SENTINEL, f"{what}: more than {self.n} lengths were written"
            assert lengths[:self.n] == want.lengths, f"{what}: lengths {lengths[:self.n]}, the emitter's are {want.lengths}"
        D.same_text(got[self.start:self.start + size], want.data, what)
        outside = np.concatenate([got[:self.start], got[self.start + size:]])
        assert (outside == FILL).all(), f"{what}: {int((outside != FILL).sum())} bytes outside the output's {size} were written"
        if want.texts:
            self.texts = [got[self.start + end - k:self.start + end].copy() for k, end in zip(want.lengths, np.cumsum(want.lengths))]


def show(shown, kind, slot, want, what):
    """the terminal's model follows the texts the device wrote: after each it shows the frame"""
    for text, (_, frame, key) in zip(slot.texts, want.texts):
        if key:
            shown.terminal = TERMINAL[kind](frame.shape[1], frame.shape[0])
        shown.terminal.feed(text).shows(frame, what)


# ---- the raw calls: host memory the test owns, overwritten as soon as the call returns ----

def _ok(rc, what):
    assert rc == hip.TRT_OK, f"{what}: {hip.ERRORS.get(rc, rc)}: {hip.lib().trt_last_error().decode()}"


def call_render(handle, step, frames, slot, expect_rc=hip.TRT_OK):
    """the step's entry through hip.lib() with a Camera (or an array of them) and a trt_rowset of the test's own; both are overwritten -- NaNs
    and zeros -- as soon as the call has returned"""
    kind, batch = KIND_OF[step.entry]
    rows = hip.RowSet.whole(frames.w, frames.h)
    n = len(step.cams)
    cams = (L.Camera * n)()
    for k, c in enumerate(step.cams):
        a = np.ascontiguousarray(frames.camera(c), dtype=np.float64)
        C.memmove(C.byref(cams[k]), a.ctypes.data, 120)
    args = [handle, C.addressof(cams), n] if batch else [handle, C.cast(cams, C.POINTER(L.Camera))]
    args += [C.byref(rows), frames.bounce, frames.spp, slot.ptr, slot.capacity]
    if kind in DELTA:
        args.append(slot.lengths_ptr)
    rc = getattr(hip.lib(), step.entry)(*args)
    C.memset(C.byref(cams), 0xFF, C.sizeof(cams))  # every double a NaN
    C.memset(C.byref(rows), 0, C.sizeof(rows))
    if expect_rc == hip.TRT_OK:
        _ok(rc, step.entry)
    else:
        assert rc == expect_rc, f"{step.entry}: {hip.ERRORS.get(rc, rc)} for {hip.ERRORS[expect_rc]}"


def slots_for(steps, frames):
    out = []
    for k, step in enumerate(steps):
        kind, _ = KIND_OF[step.entry]
        n = len(step.cams)
        out.append(Slot(capacity_of(kind, frames.w, frames.h, n), n if kind in DELTA else 0, 0 if kind == "doubles" else k % 4))
    return out


Outcome = collections.namedtuple("Outcome", "seconds gates closed")


def run_steps(handles, streams, steps, frames, gate_for=None, before_sync=None):
    """The caller protocol for render entries.  handles[i] renders on streams[i] (torch streams).  With gate_for (ms) a gate goes in front on every
    stream; behind it, on the stream: outputs and guards filled with 0xA5, the call, the snapshot, the scribble.  One synchronisation, at the
    very end; then every snapshot is held against the oracle.  Returns (host seconds over the calls, the gates, whether every gate was
    still closed when the last call had returned)."""
    import torch
    lib = hip.lib()
    slots = slots_for(steps, frames)
    torch.cuda.synchronize()
    for h in handles:
        _ok(lib.trt_ansi_delta_reset(h), "trt_ansi_delta_reset")
    gates = [Gate(s, gate_for) for s in streams] if gate_for else []
    t0 = time.perf_counter()
    for step, slot in zip(steps, slots):
        with torch.cuda.stream(streams[step.who]):
            slot.arm()
            if step.reset:
                _ok(lib.trt_ansi_delta_reset(handles[step.who]), "trt_ansi_delta_reset")
            call_render(handles[step.who], step, frames, slot)
            slot.take()
    seconds = time.perf_counter() - t0
    extra = before_sync() if before_sync else None
    closed = all(g.closed() for g in gates)
    for s in streams:
        s.synchronize()
    shown = [Shown() for _ in handles]
    for k, (step, slot) in enumerate(zip(steps, slots)):
        kind, _ = KIND_OF[step.entry]
        what = f"call {k}, {step.entry} of camera(s) {step.cams}" + (", gated" if gate_for else ", warm-up")
        if step.reset:
            shown[step.who].reset()
        want = expected(kind, frames, step.cams, shown[step.who])
        slot.check(want, what)
        if want.texts:
            show(shown[step.who], kind, slot, want, what)
    if extra:
        extra()
    return Outcome(seconds, gates, closed)
