"""The sixel image's device entries (trt_render_device_sixel, trt_sixel_from_rgb8_device) under the asynchronous contract of
include/trt_hip.h, WHILE THE STREAM IS KNOWN TO BE BACKED UP: tests/test_stream_order.py's protocol -- a gate in front, outputs and lengths
armed, snapshotted and scribbled over on the stream, host memory overwritten as soon as a call returns, one synchronisation at the very end
-- through the machinery of tests/stream_order_support.py, with this format's expected bytes (the host emitter's of the oracle's frame).

tests/test_stream_order.py demands a scenario for every asynchronous entry the header declares and reads the table of scenarios from
stream_order_support.  That module is left as it is: THIS module adds its scenario to the table when it is imported, which the collection
of the suite does before any test runs, as tests/test_kitty_stream_order.py does.  (Run by itself, tests/test_stream_order.py does not see
it.)"""
import ctypes as C
import time

import numpy as np
import pytest

import stream_order_support as O
from stream_order_support import HEIGHT, W, Format, Frames, Gate, Slot, Step
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import layout as L

# images between other kinds, so that one kind's ordered mean arms the queue for the next launch, then the formatting alone from bytes that
# arrive on the stream; every output at another alignment
RUN = (Step("trt_render_device_sixel", (0,)), Step("trt_render_device", (1,)), Step("trt_render_device_sixel", (2,)),
       Step("trt_render_device_rgb8", (3,)), Step("trt_render_device_sixel", (1,)))
FORMATTING = (Format("trt_sixel_from_rgb8_device", 1),)

O.KIND_OF.update({"trt_render_device_sixel": ("sixel", False)})
O.SCENARIOS["the sixel image"] = RUN + FORMATTING


def test_the_sixel_entries_are_in_the_table_of_scenarios():
    declared = O.asynchronous_entries()
    mine = {"trt_render_device_sixel", "trt_sixel_from_rgb8_device"}
    assert mine == {name for name in declared if "sixel" in name} and mine <= O.covered_entries()
    assert not [name for name in declared if name not in O.covered_entries()]


def _want(rgb):
    text = host.emitter_sixel_rgb8(rgb)
    return O.Want(text, [int(text.size)], None)


def _call_sixel(handle, step, frames, slot):
    """O.call_render's protocol for the entry that takes a capacity and the length's device address: a Camera and a trt_rowset of the test's
    own, overwritten -- NaNs and zeros -- as soon as the call has returned"""
    rows = hip.RowSet.whole(frames.w, frames.h)
    cam = L.Camera()
    a = np.ascontiguousarray(frames.camera(step.cams[0]), dtype=np.float64)
    C.memmove(C.byref(cam), a.ctypes.data, 120)
    rc = hip.lib().trt_render_device_sixel(handle, C.byref(cam), C.byref(rows), frames.bounce, frames.spp, slot.ptr, slot.capacity, slot.lengths_ptr)
    C.memset(C.byref(cam), 0xFF, C.sizeof(cam))  # every double a NaN
    C.memset(C.byref(rows), 0, C.sizeof(rows))
    O._ok(rc, step.entry)


@pytest.mark.gpu
def test_images_between_other_kinds_and_the_formatting_alone_behind_a_gate():
    import torch
    route = O.ROUTES["plain rounds"]
    frames = Frames(route.scene, route.bounce)
    rgb, old = frames.rgb(1), frames.rgb(3)
    assert not np.array_equal(rgb, old)
    real = torch.from_numpy(np.concatenate([[np.uint8(0)], rgb.reshape(-1)])).to("cuda:0")  # the frame one byte behind an aligned address
    stale = torch.from_numpy(np.concatenate([[np.uint8(0)], old.reshape(-1)])).to("cuda:0")
    room = hip.sixel_capacity(W, HEIGHT)
    lib = hip.lib()
    with hip.Context(0) as ctx:
        O.configure(ctx, route)
        stream = torch.cuda.Stream(device="cuda:0")
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            kinds = [O.KIND_OF[step.entry][0] for step in RUN]
            slots = [Slot(room, 1, k % 4) if kind == "sixel" else Slot(O.capacity_of(kind, W, HEIGHT, 1), 0, 0 if kind == "doubles" else k % 4)
                     for k, kind in enumerate(kinds)]
            alone, buf = Slot(room, 1, 3), stale.clone()
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            for step, slot, kind in zip(RUN, slots, kinds):
                with torch.cuda.stream(stream):
                    slot.arm()
                    if kind == "sixel":
                        _call_sixel(ctx._h, step, frames, slot)
                    else:
                        O.call_render(ctx._h, step, frames, slot)
                    slot.take()
            with torch.cuda.stream(stream):
                buf.copy_(real)
                alone.arm()
                O._ok(lib.trt_sixel_from_rgb8_device(ctx._h, buf.data_ptr() + 1, W, HEIGHT, alone.ptr, room, alone.lengths_ptr), FORMATTING[0].entry)
                alone.take()
                buf.fill_(0x77)
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            tag = ", gated" if gate_for else ", warm-up"
            for k, (step, slot, kind) in enumerate(zip(RUN, slots, kinds)):
                want = _want(frames.rgb(step.cams[0])) if kind == "sixel" else O.expected(kind, frames, step.cams, None)
                slot.check(want, f"call {k}, {step.entry} of camera {step.cams}" + tag)
            alone.check(_want(rgb), FORMATTING[0].entry + tag)
            return O.Outcome(seconds, gates, closed)

        warm = once(None)
        out = once(O.gate_ms(warm.seconds))
        O.report("sixel images and their formatting alone", warm.seconds, out.gates[0], out.closed)
        assert out.closed, f"the gate of {out.gates[0].achieved_ms():.1f} ms opened before the last call had returned -- an entry waited for the device"
