"""The 256-colour texts' device entries (trt_render_device_ansi256[_half], trt_render_device_batch_ansi256[_half],
trt_ansi256[_half]_from_rgb8_device, trt_xterm256_from_rgb8_device) under the asynchronous contract of include/trt_hip.h, WHILE THE STREAM
IS KNOWN TO BE BACKED UP: tests/test_stream_order.py's protocol -- a gate in front, outputs armed, snapshotted and scribbled over on the
stream, host memory overwritten as soon as a call returns, one synchronisation at the very end -- through the machinery of
tests/stream_order_support.py, with these formats' expected bytes (the host emitters' of the oracle's frame).

tests/test_stream_order.py demands a scenario for every asynchronous entry the header declares and reads the table of scenarios from
stream_order_support.  That module is left as it is: THIS module adds its scenario to the table when it is imported, which the collection
of the suite does before any test runs, as tests/test_kitty_stream_order.py does.  (Run by itself, tests/test_stream_order.py does not see
it.)"""
import time

import numpy as np
import pytest

import ansi256_support as A
import stream_order_support as O
from stream_order_support import HEIGHT, W, Format, Frames, Gate, Slot, Step
from terminalraytracer_amd import hip, host

# texts between other kinds, so that one kind's ordered mean arms the queue for the next kind's launch; every output at another alignment
RUN = (Step("trt_render_device_ansi256", (0,)), Step("trt_render_device", (1,)), Step("trt_render_device_batch_ansi256_half", (2, 3, 0)),
       Step("trt_render_device_ansi256_half", (1,)), Step("trt_render_device_rgb8", (2,)), Step("trt_render_device_batch_ansi256", (3, 0, 1)),
       Step("trt_render_device_ansi256", (3,)))
FORMATTING = (Format("trt_ansi256_from_rgb8_device", 1), Format("trt_ansi256_half_from_rgb8_device", 1), Format("trt_xterm256_from_rgb8_device", 1))

O.KIND_OF.update({"trt_render_device_ansi256": ("ansi256", False), "trt_render_device_ansi256_half": ("ansi256_half", False),
                  "trt_render_device_batch_ansi256": ("ansi256", True), "trt_render_device_batch_ansi256_half": ("ansi256_half", True)})
O.SCENARIOS["the 256-colour texts"] = RUN + FORMATTING
MINE = {"ansi256": False, "ansi256_half": True}  # kind: half-block cells


def test_the_256_colour_entries_are_in_the_table_of_scenarios():
    declared = O.asynchronous_entries()
    mine = {step.entry for step in RUN + FORMATTING if "256" in step.entry}
    assert len(mine) == 7 and mine <= set(declared) and mine <= O.covered_entries()
    assert mine == {name for name in declared if "256" in name}
    assert not [name for name in declared if name not in O.covered_entries()]


def _capacity(kind, n):
    return n * hip.ansi256_bytes(W, HEIGHT, MINE[kind]) if kind in MINE else O.capacity_of(kind, W, HEIGHT, n)


def _expected(kind, frames, cams):
    if kind in MINE:
        return O.Want(np.concatenate([host.emitter_ansi256_rgb8(frames.rgb(c), MINE[kind]) for c in cams]), None, None)
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
def test_a_run_of_256_colour_texts_between_other_kinds_behind_a_gate():
    import torch
    route = O.ROUTES["plain rounds"]
    frames = Frames(route.scene, route.bounce)
    with hip.Context(0) as ctx:
        O.configure(ctx, route)
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            kinds = [O.KIND_OF[step.entry][0] for step in RUN]
            slots = [Slot(_capacity(kind, len(step.cams)), 0, 0 if kind == "doubles" else (k + 1) % 4) for k, (step, kind) in enumerate(zip(RUN, kinds))]
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            for step, slot in zip(RUN, slots):
                with torch.cuda.stream(stream):
                    slot.arm()
                    O.call_render(ctx._h, step, frames, slot)
                    slot.take()
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            for k, (step, slot, kind) in enumerate(zip(RUN, slots, kinds)):
                slot.check(_expected(kind, frames, step.cams), f"call {k}, {step.entry} of camera(s) {step.cams}" + (", gated" if gate_for else ", warm-up"))
            return O.Outcome(seconds, gates, closed)

        _gated("a run of 256-colour texts", once)


@pytest.mark.gpu
def test_formatting_alone_behind_a_gate():
    """the three *_from_rgb8_device entries from a buffer whose real contents arrive on the stream behind the gate and are scribbled over
    behind the calls"""
    import torch
    frames = Frames("demo", 3)
    rgb, old = frames.rgb(1), frames.rgb(3)
    assert not np.array_equal(rgb, old)
    real = torch.from_numpy(np.concatenate([[np.uint8(0)], rgb.reshape(-1)])).to("cuda:0")  # the frame one byte behind an aligned address
    stale = torch.from_numpy(np.concatenate([[np.uint8(0)], old.reshape(-1)])).to("cuda:0")
    wants = [O.Want(host.emitter_ansi256_rgb8(rgb), None, None), O.Want(host.emitter_ansi256_rgb8(rgb, half=True), None, None),
             O.Want(A.search(rgb).astype(np.uint8).reshape(-1), None, None)]
    lib = hip.lib()
    with hip.Context(0) as ctx:
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            buf = stale.clone()
            slots = [Slot(int(want.data.size), 0, 3 - k) for k, want in enumerate(wants)]
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                buf.copy_(real)
                for slot in slots:
                    slot.arm()
                O._ok(lib.trt_ansi256_from_rgb8_device(ctx._h, buf.data_ptr() + 1, W, HEIGHT, slots[0].ptr), FORMATTING[0].entry)
                O._ok(lib.trt_ansi256_half_from_rgb8_device(ctx._h, buf.data_ptr() + 1, W, HEIGHT, slots[1].ptr), FORMATTING[1].entry)
                O._ok(lib.trt_xterm256_from_rgb8_device(ctx._h, buf.data_ptr() + 1, W * HEIGHT, slots[2].ptr), FORMATTING[2].entry)
                for slot in slots:
                    slot.take()
                buf.fill_(0x77)
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            for slot, want, step in zip(slots, wants, FORMATTING):
                slot.check(want, step.entry + (", gated" if gate_for else ", warm-up"))
            return O.Outcome(seconds, gates, closed)

        _gated("formatting 256-colour texts alone", once)
