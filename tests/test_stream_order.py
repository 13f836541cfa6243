"""The asynchronous contract of include/trt_hip.h -- every device-resident entry is "asynchronous on the context's stream" -- held against
the CPU oracle and the sequential host emitters WHILE THE STREAM IS KNOWN TO BE BACKED UP.

The rest of the suite drains the device around almost every call, so a kernel on the wrong stream, a missing guard synchronisation, a host
argument read after the call has returned or a needless host wait would pass it.  Here a GATE -- a bounded delay (stream_order_support.Gate)
-- is enqueued in front of a scenario: everything the scenario enqueues stays queued until the host has issued all of it, and an ordering
mistake shows as wrong bytes whatever the timing.  Every scenario first runs un-gated (the warm-up grows the buffers, its outputs are
checked too); its host time E sizes the gate, max(20 E, 50 ms), at most 500 ms.

The caller keeps to one protocol (stream_order_support.run_steps): before the gate the inputs hold a valid but different frame and the
outputs other bytes; behind the gate, on the stream, the real inputs are copied in, outputs and guards are filled with 0xA5, the calls are
made, and after each call the output is copied to a snapshot and scribbled over at once; host memory given to a call (Camera, trt_rowset,
the cameras of a batch, refraction indices, a scene's arrays) is overwritten as soon as the call returns.  One synchronisation at the very
end; then every snapshot equals the expected bytes bit for bit, the 64-bit lengths are the emitter's, every guard byte is intact.  The
expected bytes never come from the device.

KNOWN LIMIT.  A kernel that escapes to a stream which shares the gated stream's hardware queue is held back with it and is masked in that
run.  Every route runs on a user stream, and the first half of the run also on the context's own and on its CU-masked stream: a
mitigation, not a proof."""
import ctypes as C
import time

import numpy as np
import pytest

import ansi_delta_batch_support as B
import ansi_delta_support as D
import stream_order_support as O
import support as T
from stream_order_support import HEIGHT, W, Frames, Gate, Slot, Step
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S


def test_every_asynchronous_entry_of_the_header_has_a_scenario():
    """an entry added to include/trt_hip.h without a line in the scenario table fails here, without a GPU"""
    declared = O.asynchronous_entries()
    assert len(declared) >= 19 and "trt_quantize_device" in declared and "trt_render_device_batch_ansi_delta_half" in declared, declared
    missing = [name for name in declared if name not in O.covered_entries()]
    assert not missing, f"no scenario of tests/stream_order_support.py calls {missing}"
    assert set(O.KIND_OF) == {n for n in declared if n.startswith("trt_render_device")}
    for name, reason in O.WAITS.items():  # an entry marked "waits" is a declared one and says why
        assert name in declared and reason


gpu = pytest.mark.gpu


def _user_stream():
    import torch
    return torch.cuda.Stream(device="cuda:0")


def _gated(name, once):
    """the warm-up, then the same behind a gate sized by the warm-up's host time; the gate must still be closed when the last call has returned"""
    warm = once(None)
    out = once(O.gate_ms(warm.seconds))
    O.report(name, warm.seconds, out.gates[0], out.closed)
    assert out.closed, f"{name}: the gate of {out.gates[0].achieved_ms():.1f} ms opened before the last call had returned -- an entry waited for the device"


# ---- 1. formatting and quantising alone ----

@gpu
def test_formatting_alone_behind_a_gate():
    """trt_quantize_device, the two whole texts, the two delta texts and both chains of three from buffers whose real contents arrive on the stream
    behind the gate and are scribbled over behind every call; back to back, so that consecutive delta calls share the tile sums"""
    import torch
    frames = Frames("demo", 3)
    rgb = [frames.rgb(c) for c in range(4)]
    size = rgb[0].size
    real_px = torch.from_numpy(np.array(frames.px(0))).to("cuda:0")
    real_rgb = torch.from_numpy(np.concatenate([[np.uint8(0)]] + [f.reshape(-1) for f in rgb])).to("cuda:0")  # frame k one byte behind k * 2613
    old_px = torch.from_numpy(np.array(frames.px(1))).to("cuda:0")
    old_rgb = torch.from_numpy(np.concatenate([[np.uint8(0)]] + [rgb[(k + 2) % 4].reshape(-1) for k in range(4)])).to("cuda:0")
    full, half = B.KINDS["full"], B.KINDS["half"]
    wants = {"trt_quantize_device": O.Want(rgb[0].reshape(-1), None, None),
             "trt_ansi_from_rgb8_device": O.Want(D.full_text(rgb[1]), None, None),
             "trt_ansi_half_from_rgb8_device": O.Want(host.emitter_half_rgb8(rgb[2]), None, None)}
    for entry, kind, shown, nxt in (("trt_ansi_delta_from_rgb8_device", full, 0, [1]), ("trt_ansi_delta_half_from_rgb8_device", half, 1, [2]),
                                    ("trt_ansi_delta_chain_from_rgb8_device", full, 0, [1, 2, 3]), ("trt_ansi_delta_half_chain_from_rgb8_device", half, 0, [1, 2, 3])):
        texts = B.expected(kind, rgb[shown], [rgb[k] for k in nxt])
        wants[entry] = O.Want(np.concatenate(texts), [int(t.size) for t in texts], None)
        assert sum(t.size for t in texts) > 0
    capacities = {"trt_quantize_device": size, "trt_ansi_from_rgb8_device": hip.ansi_bytes(W, HEIGHT), "trt_ansi_half_from_rgb8_device": hip.ansi_half_bytes(W, HEIGHT),
                  "trt_ansi_delta_from_rgb8_device": hip.ansi_delta_capacity(W, HEIGHT), "trt_ansi_delta_half_from_rgb8_device": hip.ansi_delta_half_capacity(W, HEIGHT),
                  "trt_ansi_delta_chain_from_rgb8_device": 3 * hip.ansi_delta_capacity(W, HEIGHT),
                  "trt_ansi_delta_half_chain_from_rgb8_device": 3 * hip.ansi_delta_half_capacity(W, HEIGHT)}
    lib = hip.lib()
    with hip.Context(0) as ctx:
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)

        def once(gate_for):
            px, buf = old_px.clone(), old_rgb.clone()
            at = [buf.data_ptr() + 1 + k * size for k in range(4)]
            slots = [Slot(capacities[f.entry], f.n if "delta" in f.entry else 0, k % 4) for k, f in enumerate(O.FORMATTING)]
            torch.cuda.synchronize()
            gates = [Gate(stream, gate_for)] if gate_for else []
            t0 = time.perf_counter()
            with torch.cuda.stream(stream):
                for f, slot in zip(O.FORMATTING, slots):
                    px.copy_(real_px)
                    buf.copy_(real_rgb)
                    slot.arm()
                    h, cap = ctx._h, slot.capacity
                    rc = {"trt_quantize_device": lambda: lib.trt_quantize_device(h, px.data_ptr(), W * HEIGHT, slot.ptr),
                          "trt_ansi_from_rgb8_device": lambda: lib.trt_ansi_from_rgb8_device(h, at[1], W, HEIGHT, slot.ptr),
                          "trt_ansi_half_from_rgb8_device": lambda: lib.trt_ansi_half_from_rgb8_device(h, at[2], W, HEIGHT, slot.ptr),
                          "trt_ansi_delta_from_rgb8_device": lambda: lib.trt_ansi_delta_from_rgb8_device(h, at[0], at[1], W, HEIGHT, slot.ptr, cap, slot.lengths_ptr),
                          "trt_ansi_delta_half_from_rgb8_device": lambda: lib.trt_ansi_delta_half_from_rgb8_device(h, at[1], at[2], W, HEIGHT, slot.ptr, cap, slot.lengths_ptr),
                          "trt_ansi_delta_chain_from_rgb8_device": lambda: lib.trt_ansi_delta_chain_from_rgb8_device(h, at[0], at[1], 3, W, HEIGHT, slot.ptr, cap, slot.lengths_ptr),
                          "trt_ansi_delta_half_chain_from_rgb8_device": lambda: lib.trt_ansi_delta_half_chain_from_rgb8_device(h, at[0], at[1], 3, W, HEIGHT, slot.ptr, cap,
                                                                                                                               slot.lengths_ptr)}[f.entry]()
                    O._ok(rc, f.entry)
                    slot.take()
                    px.fill_(float("nan"))
                    buf.fill_(0x77)
            seconds = time.perf_counter() - t0
            closed = all(g.closed() for g in gates)
            stream.synchronize()
            for f, slot in zip(O.FORMATTING, slots):
                slot.check(wants[f.entry], f.entry + (", gated" if gate_for else ", warm-up"))
            return O.Outcome(seconds, gates, closed)

        _gated("formatting alone", once)


# ---- 2. a run of frames of every kind, once per route ----

@gpu
@pytest.mark.parametrize("route", sorted(O.ROUTES))
def test_a_run_of_frames_of_every_kind_behind_a_gate(route):
    """One context, one rowset, one user stream: doubles, bytes, both texts, keyframes and deltas of both kinds, the four batch forms, both
    batch deltas, a reset, doubles again -- back to back behind the gate.  Eye tables are rebuilt in a slot while the frame before is queued,
    batch slots stand against the context's own, one kind's ordered mean arms the queue for the next kind's launch, the delta frame
    buffers flip, and the scratch is shared by all of them."""
    r = O.ROUTES[route]
    frames = Frames(r.scene, r.bounce)
    with hip.Context(0) as ctx:
        O.configure(ctx, r)
        stream = _user_stream()
        ctx.set_stream(stream.cuda_stream)
        _gated(f"a run of frames, {route}", lambda gate_for: O.run_steps([ctx._h], [stream], O.RUN, frames, gate_for))
        if route == "decoupled rounds":
            assert ctx.render_variant()["decoupled"]
        if route == "scene image in device memory":
            assert ctx.render_image()["in_device_memory"]


# ---- 3. the context's own stream, plain and CU-masked ----

@gpu
@pytest.mark.parametrize("reserved", [0, 8])
def test_the_first_half_of_the_run_on_the_contexts_own_stream(reserved):
    """no trt_set_stream: the gate goes onto the stream trt_get_stream returns, wrapped as the header recommends; then the same on the stream
    trt_reserve_cus re-creates with a CU mask"""
    import torch
    r = O.ROUTES["plain rounds"]
    frames = Frames(r.scene, r.bounce)
    with hip.Context(0) as ctx:
        O.configure(ctx, r)
        if reserved:
            ctx.reserve_cus(reserved)
        stream = torch.cuda.ExternalStream(ctx.stream_ptr(), device=torch.device("cuda:0"))
        _gated(f"the context's own stream, {reserved} CUs reserved", lambda gate_for: O.run_steps([ctx._h], [stream], O.FIRST_HALF, frames, gate_for))
        torch.cuda.synchronize()


# ---- 4. two contexts, one scene ----

@gpu
def test_two_contexts_of_one_scene_take_turns_behind_their_gates():
    """trt_share_scene: each context on its own gated user stream and in its own eye slot of the shared tables, single-frame calls with
    different cameras taking turns; both contexts' frames are the oracle's.  A batch of 2 on the sharer is refused with nothing enqueued."""
    r = O.ROUTES["decoupled rounds"]
    frames = Frames(r.scene, r.bounce)
    with hip.Context(0) as a, hip.Context(0) as b:
        O.configure(a, r)
        b.set_compaction(r.compaction)
        b.share_scene(a)
        streams = [_user_stream(), _user_stream()]
        a.set_stream(streams[0].cuda_stream)
        b.set_stream(streams[1].cuda_stream)
        refused = Step("trt_render_device_batch_rgb8", (0, 1), 1)

        def once(gate_for):
            import torch
            slot = Slot(O.capacity_of("rgb8", W, HEIGHT, 2))
            torch.cuda.synchronize()

            def before_sync():
                with torch.cuda.stream(streams[1]):
                    slot.arm()
                    O.call_render(b._h, refused, frames, slot, expect_rc=O.CAPACITY)
                    slot.take()
                return lambda: slot.untouched() or pytest.fail("the refused batch wrote to its output")

            return O.run_steps([a._h, b._h], streams, O.SHARED, frames, gate_for, before_sync)

        _gated("two contexts, one scene", once)


# ---- 5. calls that may have to wait ----

REFRACTORS = tuple(1.5 if k % 3 == 0 else 0.0 for k in range(24))
OTHER_REFRACTORS = tuple(1.3 if k % 2 == 0 else 0.0 for k in range(24))


def _private_scene(name):
    """the scene in arrays of the test's own, to be zeroed once trt_set_scene has returned"""
    sc = O.scene(name)
    return S.SceneData(sc.spheres.copy(), sc.ground.copy(), sc.dir_lights.copy(), sc.point_lights.copy(), sc.camera.copy(), sc.sky.copy())


def _waiting_calls(ctx, streams, gate_for):
    """Every frame marked GATED below is queued behind a gate of its own, and the call behind it rewrites or replaces something that frame still
    reads.  A gated frame repeats the state of the frame before it, so that nothing in its own call drains the gate.  The first three steps use
    cameras whose pixels measure 1/16 at every size, so that each leans on ONE guard:
       A (67 x 13, 3 rays per pixel), then the same at 2 rays per pixel: prepare_jitter rewrites its table, which does not grow, behind its
         synchronisation -- nothing else protects A;
       then a frame of 63 x 17: as many axis values, so prepare_axes rewrites its table in place behind its synchronisation, nothing else;
       then a batch of three of that size: launch_production's sample scratch grows behind its synchronisation;
       B at 71 x 17 and 5 rays per pixel: jitter, axes and scratch all change (the first guard met drains the stream);
       C, then trt_set_path_grids: its synchronisation in front of the rebuilt candidate tables; D reads the new ones;
       E, then trt_set_refraction with refractors: F is the refractive oracle's; G (refractive), then trt_set_refraction with OTHER indices,
         uploaded into the same buffer behind the entry's synchronisation -- nothing else protects G; then without: opaque again;
       I, then trt_set_scene of another scene: its synchronisation in front of the primitives' upload and the tables' build; J is that scene's;
       K, then trt_set_stream to a second stream, which synchronises the first: L on the second; M, and back: N on the first;
       P, a delta text, then Q, the delta texts of a batch of three, and R, another batch: render_device_delta synchronises before the frame
         buffer it renders into grows (the first guard Q meets; launch_ansi_delta's, before the tile sums grow, and the scratch's follow it);
       S on the reference-order kernel, whose bytes go through the context's framebuffer d_fb, then trt_render_host of 83 x 19, which grows d_fb
         with no synchronisation of the library's in front: hipFree's own device-wide wait is what protects S.
    Host memory -- cameras, rowsets, the refraction indices, the scene's arrays -- is overwritten as soon as each call has returned.
    Returns the host seconds of the frame in front of each waiting call, for the gates."""
    import torch
    lib = hip.lib()
    a3, a2 = Frames("synth24", 3, spp=3, screen=16), Frames("synth24", 3, spp=2, screen=16)
    b2 = Frames("synth24", 3, spp=2, w=63, h=17, screen=16)
    large = Frames("synth24", 3, spp=5, w=71, h=17)
    refr, other = Frames("synth24", 3, spp=5, w=71, h=17, ior=REFRACTORS), Frames("synth24", 3, spp=5, w=71, h=17, ior=OTHER_REFRACTORS)
    demo, wide = Frames("demo", 3, spp=5, w=71, h=17), Frames("demo", 3, spp=5, w=83, h=19)
    assert a2.w + a2.h == b2.w + b2.h
    doubles, rgb8, delta, batch = "trt_render_device", "trt_render_device_rgb8", "trt_render_device_ansi_delta", "trt_render_device_batch_rgb8"
    batch_delta = "trt_render_device_batch_ansi_delta"
    checks, seconds, gates, host_frames = [], [], [], []
    shown = O.Shown()
    private = _private_scene("demo")
    sc = private.as_scene()

    def refract(indices):
        def call():
            ior = np.array(indices)
            O._ok(lib.trt_set_refraction(ctx._h, ior.ctypes.data, ior.size), "trt_set_refraction")
            ior[:] = np.nan
        return call

    def another_scene():
        O._ok(lib.trt_set_scene(ctx._h, C.byref(sc)), "trt_set_scene")
        for a in (private.spheres, private.ground, private.dir_lights, private.point_lights, private.sky):
            a[...] = 0
        C.memset(C.byref(sc), 0, C.sizeof(sc))

    def host_frame():
        got = ctx.render_host(wide.camera(3), hip.RowSet.whole(wide.w, wide.h), wide.bounce, wide.spp)
        host_frames.append((got, wide.px(3), "trt_render_host of 83 x 19 behind a queued frame of the reference-order kernel"))

    GATED = True
    plan = [(doubles, (3,), a3, 0),          # the context's first frame grows its buffers and drains the stream on the way: not gated
            (doubles, (0,), a3, 0, GATED),   # A
            (rgb8, (1,), a2, 0),             # the jitter table alone
            (doubles, (2,), a2, 0, GATED),
            (rgb8, (3,), b2, 0),             # the axes alone
            (doubles, (0,), b2, 0, GATED),
            (batch, (1, 2, 3), b2, 0),       # the scratch alone
            (doubles, (1,), b2, 0, GATED),
            (rgb8, (1,), large, 0),          # B
            (doubles, (2,), large, 0, GATED),  # C
            lambda: O._ok(lib.trt_set_path_grids(ctx._h, 16, 8), "trt_set_path_grids"),
            (rgb8, (3,), large, 0),          # D
            (doubles, (0,), large, 0, GATED),  # E
            refract(REFRACTORS),
            (doubles, (1,), refr, 0),        # F
            (rgb8, (2,), refr, 0, GATED),    # G
            refract(OTHER_REFRACTORS),
            (doubles, (3,), other, 0),
            (rgb8, (0,), other, 0, GATED),
            lambda: O._ok(lib.trt_set_refraction(ctx._h, None, 0), "trt_set_refraction"),
            (doubles, (3,), large, 0),       # H
            (rgb8, (0,), large, 0, GATED),   # I
            another_scene,
            (doubles, (1,), demo, 0),        # J
            (rgb8, (2,), demo, 0, GATED),    # K
            lambda: O._ok(lib.trt_set_stream(ctx._h, streams[1].cuda_stream), "trt_set_stream"),
            (doubles, (3,), demo, 1),        # L
            (rgb8, (0,), demo, 1, GATED),    # M
            lambda: O._ok(lib.trt_set_stream(ctx._h, streams[0].cuda_stream), "trt_set_stream"),
            (doubles, (1,), demo, 0),        # N
            (delta, (2,), demo, 0),          # a keyframe and a delta, not gated: each grows the frame buffer it renders into
            (delta, (3,), demo, 0),
            (delta, (0,), demo, 0, GATED),   # P
            (batch_delta, (1, 2, 3), demo, 0),  # Q
            (batch_delta, (0, 1, 2), demo, 0),  # R
            lambda: O._ok(lib.trt_set_kernel(ctx._h, hip.Context.REFERENCE_ORDER), "trt_set_kernel"),
            (rgb8, (2,), demo, 0),           # d_fb at this size, with nothing queued
            (rgb8, (1,), demo, 0, GATED),    # S
            host_frame]
    slots = {}
    for k, item in enumerate(plan):  # every buffer before the first gate: an allocation in between would drain the device
        if not callable(item):
            kind, _ = O.KIND_OF[item[0]]
            slots[k] = Slot(O.capacity_of(kind, item[2].w, item[2].h, len(item[1])), len(item[1]) if kind in O.DELTA else 0, 0 if kind == "doubles" else k % 4)
    torch.cuda.synchronize()
    for k, item in enumerate(plan):
        if callable(item):
            item()
            continue
        entry, cams, frames, stream = item[:4]
        gated = len(item) > 4
        kind, _ = O.KIND_OF[entry]
        if gated and gate_for:
            gates.append(Gate(streams[stream], gate_for[len(seconds)]))
        t0 = time.perf_counter()
        with torch.cuda.stream(streams[stream]):
            slots[k].arm()
            O.call_render(ctx._h, Step(entry, cams), frames, slots[k])
            slots[k].take()
        if gated:
            seconds.append(time.perf_counter() - t0)
        checks.append((slots[k], kind, O.expected(kind, frames, cams, shown), f"frame {len(checks)} ({entry} of camera(s) {cams}, {frames.key})"))
    for s in streams:
        s.synchronize()
    for slot, kind, want, what in checks:
        slot.check(want, what + (", gated" if gate_for else ", warm-up"))
        if want.texts:
            O.show(shown, kind, slot, want, what)
    for got, want, what in host_frames:
        assert np.array_equal(T.bits(got), T.bits(want)), what
    assert len(host_frames) == 1
    return seconds, gates


@gpu
def test_calls_that_may_have_to_wait_leave_every_frame_what_it_was_called_for():
    """the only test of the guard synchronisations: _waiting_calls says which guard each step leans on.  The warm-up runs on a context of its
    own, so that the gated context still has every buffer to grow; only correctness is asserted, these calls may wait"""
    for gated in (False, True):
        with hip.Context(0) as ctx:
            ctx.set_scene(O.scene("synth24"))
            streams = [_user_stream(), _user_stream()]
            ctx.set_stream(streams[0].cuda_stream)
            if not gated:
                warm, _ = _waiting_calls(ctx, streams, None)
            else:
                seconds, gates = _waiting_calls(ctx, streams, [O.gate_ms(s) for s in warm])
                assert len(gates) == len(warm) == len(seconds)
                print("stream order: calls that may have to wait: " +
                      ", ".join(f"E = {e * 1e3:.3f} ms / gate {g.achieved_ms():.1f} ms" for e, g in zip(warm, gates)))


# ---- 7. the harness can see a violation ----

@gpu
def test_a_caller_that_formats_on_another_stream_gets_the_old_frame():
    """The negative control: a caller's mistake on plain buffers, nothing of the library changed and nothing faults.  The producer's write of
    the new frame is queued behind the gate on one stream; trt_ansi_from_rgb8_device is issued from a context on another, free-running
    stream, and only that stream is synchronised: while the gate is still closed the text is exactly the emitter's of the OLD frame."""
    import torch
    frames = Frames("demo", 3)
    old, new = frames.rgb(0), frames.rgb(2)
    assert not np.array_equal(old, new)
    rgb = torch.from_numpy(np.array(old).reshape(-1)).to("cuda:0")
    fresh = torch.from_numpy(np.array(new).reshape(-1)).to("cuda:0")
    slot = Slot(hip.ansi_bytes(W, HEIGHT))
    probe = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    producer = _user_stream()
    with hip.Context(0) as ctx:
        ctx.ansi_from_rgb8(rgb.data_ptr(), W, HEIGHT, slot.ptr)  # first use of the kernel, before the gate
        ctx.synchronize()
        torch.cuda.synchronize()
        gate = Gate(producer, 400.0)
        with torch.cuda.stream(producer):
            rgb.copy_(fresh)
        free = None
        for _ in range(8):  # with few hardware queues two streams can share one and serialise: look for one that runs while the gate is closed
            candidate = _user_stream()
            done = torch.cuda.Event()
            with torch.cuda.stream(candidate):
                probe.fill_(1)
                done.record()
            until = time.perf_counter() + 0.02
            while not done.query() and time.perf_counter() < until:
                pass
            if done.query():
                free = candidate
                break
        if free is None:
            producer.synchronize()
            pytest.skip("no stream of 8 completed a one-element fill while the gate was closed: every stream shares the gated stream's hardware queue")
        ctx.set_stream(free.cuda_stream)
        with torch.cuda.stream(free):
            slot.arm()
            ctx.ansi_from_rgb8(rgb.data_ptr(), W, HEIGHT, slot.ptr)
            slot.take()
        free.synchronize()
        closed = gate.closed()
        with torch.cuda.stream(free):
            snap = slot.snap.cpu().numpy()
        producer.synchronize()
        assert closed, f"the gate of {gate.achieved_ms():.1f} ms opened before the text was complete"
        D.same_text(snap[slot.start:slot.start + slot.capacity], D.full_text(old), "the text of a frame whose producer is still queued")
        assert np.array_equal(rgb.cpu().numpy(), new.reshape(-1))
        print(f"stream order: negative control: gate {gate.achieved_ms():.1f} ms, the unordered call saw the old frame")
