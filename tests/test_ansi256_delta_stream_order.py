"""The device entries of the delta texts in the xterm 256-colour palette (trt_render_device_ansi256_delta[_half],
trt_render_device_batch_ansi256_delta[_half], trt_ansi256_delta[_half]_from_rgb8_device, trt_ansi256_delta[_half]_chain_from_rgb8_device)
under the asynchronous contract of include/trt_hip.h, WHILE THE STREAM IS KNOWN TO BE BACKED UP: tests/test_stream_order.py's protocol -- a
gate in front, outputs armed, snapshotted and scribbled over on the stream, host memory overwritten as soon as a call returns, one
synchronisation at the very end -- through the machinery of tests/stream_order_support.py, with these formats' expected bytes (the
sequential emitters' of the oracle's frames) and the model of which frame a context shows, as which of the four kinds.

tests/test_stream_order.py demands a scenario for every asynchronous entry the header declares and reads the table of scenarios from
stream_order_support.  That module is left as it is: THIS module adds its expected texts and its scenario to the tables when it is imported, which
the collection of the suite does before any test runs, as tests/test_ansi256_stream_order.py does."""
import ctypes as C
import functools
import os
import re
import time

import numpy as np
import pytest

import ansi256_delta_support as A
import stream_order_support as O
import support as T
from stream_order_support import BATCH, HEIGHT, W, Format, Frames, Gate, Slot, Step
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import layout as L

# a keyframe and a delta of either palette kind, a 24-bit delta call between them (a keyframe: the kind changed), batches that start with a
# keyframe and that continue a single frame's delta, a single frame that continues a batch; every output at another alignment
RUN = (Step("trt_render_device_ansi256_delta", (0,)), Step("trt_render_device_ansi256_delta", (1,)), Step("trt_render_device_ansi256_delta_half", (2,)),
       Step("trt_render_device_ansi256_delta_half", (3,)), Step("trt_render_device_ansi_delta", (0,)), Step("trt_render_device_ansi256_delta", (1,)),
       Step("trt_render_device_batch_ansi256_delta", (2, 3, 0)), Step("trt_render_device_batch_ansi256_delta_half", (1, 2, 3)),
       Step("trt_render_device_ansi256_delta_half", (0,)), Step("trt_render_device_ansi256_delta", (2,), 0, True))
FORMATTING = (Format("trt_ansi256_delta_from_rgb8_device", 1), Format("trt_ansi256_delta_half_from_rgb8_device", 1),
              Format("trt_ansi256_delta_chain_from_rgb8_device", BATCH), Format("trt_ansi256_delta_half_chain_from_rgb8_device", BATCH))

MINE = {"delta256": False, "delta256_half": True}  # kind: half-block cells
# (kind of output, batch form) of this family's render entries, beside stream_order_support's: that table is held to the header's `int`
# declarations by tests/test_stream_order.py, so these stand here and call_render below reads both
KIND_OF = dict(O.KIND_OF, **{"trt_render_device_ansi256_delta": ("delta256", False), "trt_render_device_ansi256_delta_half": ("delta256_half", False),
                             "trt_render_device_batch_ansi256_delta": ("delta256", True), "trt_render_device_batch_ansi256_delta_half": ("delta256_half", True)})
for _kind, _half in MINE.items():
    O.WHOLE[_kind] = functools.partial(host.emitter_ansi256_rgb8, half=_half)
    O.DELTA[_kind] = functools.partial(host.emitter_delta256_rgb8, half=_half)
    O.TERMINAL[_kind] = A.HalfTerminal if _half else A.Terminal
O.SCENARIOS["the 256-colour delta texts"] = RUN + FORMATTING


def declared_delta256_entries():
    """the asynchronous entries of this family in include/trt_hip.h, which declares the family `extern int` (its comment says why:
    stream_order_support.asynchronous_entries, which reads the `int` declarations, is held to the whole 256-colour texts' seven by
    tests/test_ansi256_stream_order.py): trt_render_device*, *_from_rgb8_device"""
    with open(os.path.join(T.ROOT, "include", "trt_hip.h")) as fh:
        names = re.findall(r"^extern\s+int\s+(trt_\w+)\s*\(", fh.read(), re.M)
    assert names and all("ansi256_delta" in n for n in names), names
    return sorted(n for n in names if n.startswith("trt_render_device") or n.endswith("_from_rgb8_device"))


def test_the_256_colour_delta_entries_are_in_the_table_of_scenarios():
    """every asynchronous entry of the family has a scenario here, every other one of the header still has its own, and the two readings of
    the header together see every entry of the kind the header declares"""
    declared = declared_delta256_entries()
    mine = {step.entry for step in RUN + FORMATTING if "256_delta" in step.entry}
    assert len(mine) == 8 and mine == set(declared) and mine <= O.covered_entries()
    assert not set(declared) & set(O.asynchronous_entries())
    assert not [name for name in O.asynchronous_entries() if name not in O.covered_entries()]
    with open(os.path.join(T.ROOT, "include", "trt_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    every = {n for n in re.findall(r"\b(trt_\w+)\s*\(", text) if n.startswith("trt_render_device") or n.endswith("_from_rgb8_device") or n == "trt_quantize_device"}
    assert every == set(declared) | set(O.asynchronous_entries()), every ^ (set(declared) | set(O.asynchronous_entries()))


def call_render(handle, step, frames, slot):
    """stream_order_support.call_render over this module's KIND_OF: the step's entry through hip.lib() with cameras and a trt_rowset of the
    test's own, both overwritten -- NaNs and zeros -- as soon as the call has returned"""
    _, batch = KIND_OF[step.entry]
    rows = hip.RowSet.whole(frames.w, frames.h)
    n = len(step.cams)
    cams = (L.Camera * n)()
    for k, c in enumerate(step.cams):
        a = np.ascontiguousarray(frames.camera(c), dtype=np.float64)
        C.memmove(C.byref(cams[k]), a.ctypes.data, 120)
    args = [handle, C.addressof(cams), n] if batch else [handle, C.cast(cams, C.POINTER(L.Camera))]
    args += [C.byref(rows), frames.bounce, frames.spp, slot.ptr, slot.capacity, slot.lengths_ptr]  # every step of RUN is a delta entry
    rc = getattr(hip.lib(), step.entry)(*args)
    C.memset(C.byref(cams), 0xFF, C.sizeof(cams))  # every double a NaN
    C.memset(C.byref(rows), 0, C.sizeof(rows))
    O._ok(rc, step.entry)


def _capacity(kind, n):
    return n * hip.ansi256_delta_capacity(W, HEIGHT, half=MINE[kind]) if kind in MINE else O.capacity_of(kind, W, HEIGHT, n)


def _user_stream():
    import torch
    return torch.cuda.Stream(device="cuda:0")


def _gated(name, once):
    warm = once(None)
    out = once(O.gate_ms(warm.seconds))
    O.report(name, warm.seconds, out.gates[0], out.closed)
    assert out.closed, f"{name}: the gate of {out.gates[0].achieved_ms():.1f} ms opened before the last call had returned -- an entry waited for the device"


@pytest.mark.gpu
def test_a_run_of_256_colour_delta_texts_behind_a_gate():
    """keyframes and deltas of the two palette kinds and a 24-bit one between them, single frames and batches continuing one another, a reset:
    lengths and bytes are the emitters' under the rules of the shown frame, and the terminals' models show every frame"""
    import torch
    route = O.ROUTES["plain rounds"]
    frames = Frames(route.scene, route.bounce)
    with hip.Context(0) as ctx:
        O.configure(ctx, route)
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            kinds = [KIND_OF[step.entry][0] for step in RUN]
            slots = [Slot(_capacity(kind, len(step.cams)), len(step.cams), (k + 1) % 4) for k, (step, kind) in enumerate(zip(RUN, kinds))]
            ctx.ansi_delta_reset()  # the warm-up left a shown frame behind
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            for step, slot in zip(RUN, slots):
                with torch.cuda.stream(stream):
                    if step.reset:
                        ctx.ansi_delta_reset()
                    slot.arm()
                    call_render(ctx._h, step, frames, slot)
                    slot.take()
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            shown = O.Shown()
            for k, (step, slot, kind) in enumerate(zip(RUN, slots, kinds)):
                what = f"call {k}, {step.entry} of camera(s) {step.cams}" + (", gated" if gate_for else ", warm-up")
                if step.reset:
                    shown.reset()
                want = O.expected(kind, frames, step.cams, shown)
                slot.check(want, what)
                O.show(shown, kind, slot, want, what)
            return O.Outcome(seconds, gates, closed)

        _gated("a run of 256-colour delta texts", once)


@pytest.mark.gpu
def test_formatting_alone_behind_a_gate():
    """the four *_from_rgb8_device entries from buffers whose real contents arrive on the stream behind the gate and are scribbled over behind
    the calls: a shown frame and a chain of three frames, each one byte behind an aligned address"""
    import torch
    frames = Frames("demo", 3)
    shown, chain = frames.rgb(0), [frames.rgb(c) for c in (1, 2, 3)][:BATCH]
    stale = np.full(shown.size, O.STALE, dtype=np.uint8)
    on_device = lambda *parts: torch.from_numpy(np.concatenate([[np.uint8(0)]] + [np.asarray(p).reshape(-1) for p in parts])).to("cuda:0")
    real_shown, real_chain = on_device(shown), on_device(*chain)
    stale_shown, stale_chain = on_device(stale), on_device(*([stale] * len(chain)))
    wants = []
    for step in FORMATTING:
        half = "_half" in step.entry
        texts = [host.emitter_delta256_rgb8(shown if b == 0 else chain[b - 1], chain[b], half=half) for b in range(step.n)]
        assert all(t.size for t in texts)
        wants.append(O.Want(np.concatenate(texts), [int(t.size) for t in texts], None))
    lib = hip.lib()
    with hip.Context(0) as ctx:
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            a, f = stale_shown.clone(), stale_chain.clone()
            slots = [Slot(step.n * hip.ansi256_delta_capacity(W, HEIGHT, half="_half" in step.entry), step.n, 3 - k) for k, step in enumerate(FORMATTING)]
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                a.copy_(real_shown)
                f.copy_(real_chain)
                for slot in slots:
                    slot.arm()
                for step, slot in zip(FORMATTING, slots):
                    entry = getattr(lib, step.entry)
                    args = (ctx._h, a.data_ptr() + 1, f.data_ptr() + 1) + ((step.n,) if "_chain_" in step.entry else ()) + (W, HEIGHT, slot.ptr, slot.capacity, slot.lengths_ptr)
                    O._ok(entry(*args), step.entry)
                for slot in slots:
                    slot.take()
                a.fill_(0x77)
                f.fill_(0x77)
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            for slot, want, step in zip(slots, wants, FORMATTING):
                slot.check(want, step.entry + (", gated" if gate_for else ", warm-up"))
            return O.Outcome(seconds, gates, closed)

        _gated("formatting 256-colour delta texts alone", once)
