"""The kitty image's device entries (trt_render_device_kitty, trt_render_device_batch_kitty, trt_kitty_from_rgb8_device) under the
asynchronous contract of include/trt_hip.h, WHILE THE STREAM IS KNOWN TO BE BACKED UP: tests/test_stream_order.py's protocol -- a gate in
front, outputs armed, snapshotted and scribbled over on the stream, host memory overwritten as soon as a call returns, one synchronisation
at the very end -- through the machinery of tests/stream_order_support.py, with this format's expected bytes (the host emitter's of the
oracle's frame).

tests/test_stream_order.py demands a scenario for every asynchronous entry the header declares and reads the table of scenarios from
stream_order_support.  That module is left as it is: THIS module adds its scenario to the table when it is imported, which the collection
of the suite does before any test runs.  (Run by itself, tests/test_stream_order.py does not see it; the scenario's steps belong in that
table once it is open for change.)"""
import time

import numpy as np
import pytest

import stream_order_support as O
from stream_order_support import HEIGHT, W, Format, Frames, Gate, Slot, Step
from terminalraytracer_amd import hip, host

# images between other kinds, so that one kind's ordered mean arms the queue for the next kind's launch; every output at another alignment
KITTY_RUN = (Step("trt_render_device_kitty", (0,)), Step("trt_render_device", (1,)), Step("trt_render_device_batch_kitty", (2, 3, 0)),
             Step("trt_render_device_rgb8", (1,)), Step("trt_render_device_kitty", (3,)))
KITTY_FORMATTING = (Format("trt_kitty_from_rgb8_device", 1),)

O.KIND_OF.update({"trt_render_device_kitty": ("kitty", False), "trt_render_device_batch_kitty": ("kitty", True)})
O.SCENARIOS["the kitty image"] = KITTY_RUN + KITTY_FORMATTING


def test_the_kitty_entries_are_in_the_table_of_scenarios():
    declared = O.asynchronous_entries()
    mine = {"trt_render_device_kitty", "trt_render_device_batch_kitty", "trt_kitty_from_rgb8_device"}
    assert mine <= set(declared) and mine <= O.covered_entries()
    assert not [name for name in declared if name not in O.covered_entries()]


def _capacity(kind, n):
    return n * hip.kitty_bytes(W, HEIGHT) if kind == "kitty" else O.capacity_of(kind, W, HEIGHT, n)


def _expected(kind, frames, cams):
    if kind == "kitty":
        return O.Want(np.concatenate([host.emitter_kitty_rgb8(frames.rgb(c)) for c in cams]), None, None)
    return O.expected(kind, frames, cams, None)


def _user_stream():
    import torch
    return torch.cuda.Stream(device="cuda:0")


def _gated(name, once):
    warm = once(None)
    out = once(O.gate_ms(warm.seconds))
    O.report(name, warm.seconds, out.gates[0], out.closed)
    assert out.closed, f"{name}: the gate of {out.gates[0].achieved_ms():.1f} ms opened before the last call had returned -- an entry waited for the device"


@pytest.mark.gpu
def test_a_run_of_images_between_other_kinds_behind_a_gate():
    import torch
    route = O.ROUTES["plain rounds"]
    frames = Frames(route.scene, route.bounce)
    with hip.Context(0) as ctx:
        O.configure(ctx, route)
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            kinds = [O.KIND_OF[step.entry][0] for step in KITTY_RUN]
            slots = [Slot(_capacity(kind, len(step.cams)), 0, 0 if kind == "doubles" else k % 4) for k, (step, kind) in enumerate(zip(KITTY_RUN, kinds))]
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            for step, slot in zip(KITTY_RUN, slots):
                with torch.cuda.stream(stream):
                    slot.arm()
                    O.call_render(ctx._h, step, frames, slot)
                    slot.take()
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            for k, (step, slot, kind) in enumerate(zip(KITTY_RUN, slots, kinds)):
                slot.check(_expected(kind, frames, step.cams), f"call {k}, {step.entry} of camera(s) {step.cams}" + (", gated" if gate_for else ", warm-up"))
            return O.Outcome(seconds, gates, closed)

        _gated("a run of kitty images", once)


@pytest.mark.gpu
def test_formatting_an_image_alone_behind_a_gate():
    """trt_kitty_from_rgb8_device from a buffer whose real contents arrive on the stream behind the gate and are scribbled over behind the call"""
    import torch
    frames = Frames("demo", 3)
    rgb, old = frames.rgb(1), frames.rgb(3)
    assert not np.array_equal(rgb, old)
    real = torch.from_numpy(np.concatenate([[np.uint8(0)], rgb.reshape(-1)])).to("cuda:0")  # the frame one byte behind an aligned address
    stale = torch.from_numpy(np.concatenate([[np.uint8(0)], old.reshape(-1)])).to("cuda:0")
    want = O.Want(host.emitter_kitty_rgb8(rgb), None, None)
    lib = hip.lib()
    with hip.Context(0) as ctx:
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            buf = stale.clone()
            slot = Slot(hip.kitty_bytes(W, HEIGHT), 0, 3)
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                buf.copy_(real)
                slot.arm()
                O._ok(lib.trt_kitty_from_rgb8_device(ctx._h, buf.data_ptr() + 1, W, HEIGHT, slot.ptr), KITTY_FORMATTING[0].entry)
                slot.take()
                buf.fill_(0x77)
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            slot.check(want, KITTY_FORMATTING[0].entry + (", gated" if gate_for else ", warm-up"))
            return O.Outcome(seconds, gates, closed)

        _gated("formatting an image alone", once)
