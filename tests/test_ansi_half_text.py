"""The terminal's half-block text written on the device (trt_render_device_ansi_half, trt_render_device_batch_ansi_half,
trt_render_host_ansi_half, trt_render_host_batch_ansi_half, trt_render_frame_ansi_half, trt_ansi_half_from_rgb8_device): behind the
production kernel the pass that sums a pixel's samples forms BOTH pixels of a character cell, casts them to the emitter's bytes, formats
the eighteen digits and stores the text itself, a wave per hip.ANSI_HALF_WAVE_WORDS aligned 32-bit words (csrc/trt_ansi_half.h,
trt_ansi_half.hpp).  The expected bytes never come from the library's device route: they are the sequential host emitter's
(host.emitter_half_rgb8, which tests/test_ansi_half_layout.py holds against a formatter of its own and literals) of T.oracle_rgb8 -- the
CPU checker's (int)(c*255) -- of the oracle's double frame."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import support as T
from support import STORE, DeviceBytes, anim_cameras, owned_rows, same_bytes, same_text
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4
HOME, CELL, END = 6, 39, 5


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.enable_counters(False)
        c.set_kernel(hip.Context.PRODUCTION)
        c.set_scratch_fill(False)
        c.set_scene_image(-1)
        c.set_path_patches(-1)
        c.set_compaction(-1)


@functools.lru_cache(maxsize=None)
def scene(kind):
    cam = anim_cameras([0], 160, 48)[0]
    if kind == "demo":
        return S.demo_scene(T.sky("synth"), cam)
    return S.synth_scene({"synth32": 32, "synth64": 64}[kind], T.sky("synth"), cam, seed=11)


def half_text(rgb):
    """the host emitter's half-block text of a frame of bytes [rows, w, 3]"""
    rows, w, _ = rgb.shape
    text = host.emitter_half_rgb8(rgb)
    assert text.size == HOME + (CELL * w + END) * ((rows + 1) // 2) == hip.ansi_half_bytes(w, rows)
    return text


def full_text(rgb):
    rows, w, _ = rgb.shape
    e = host.Emitter(w, rows)
    try:
        e.patch_rgb8(rgb)
        return np.frombuffer(e.bytes(), dtype=np.uint8).copy()
    finally:
        e.close()


@functools.lru_cache(maxsize=None)
def oracle(kind, w, h, index, b, spp):
    """(the oracle's double frame, its bytes by the checker's cast, the emitter's half-block text of those, (path rays, shadow rays)) --
    computed once, never written to"""
    px, st = T.oracle_render(scene(kind).with_camera(anim_cameras([index], w, h)[0]), w, h, b, spp)
    rgb = T.oracle_rgb8(px)
    text = half_text(rgb)
    px.flags.writeable = rgb.flags.writeable = text.flags.writeable = False
    return px, rgb, text, (st.path_rays, st.shadow_rays)


def device_half(ctx, cam, w, h, b, spp, offset=0, rows=None, what=""):
    rows = rows or hip.RowSet.whole(w, h)
    n = hip.ansi_half_bytes(w, owned_rows(rows))
    mem = DeviceBytes(n, offset)
    ctx.render_device_ansi_half(cam, rows, b, spp, mem.ptr, n)
    return mem.read(ctx, what)


def batch_half(ctx, cams, w, h, b, spp, offset=0, what=""):
    n = len(cams) * hip.ansi_half_bytes(w, h)
    mem = DeviceBytes(n, offset)
    ctx.render_batch_ansi_half(cams, hip.RowSet.whole(w, h), b, spp, mem.ptr, n)
    return mem.read(ctx, what).reshape(len(cams), -1)


def device_full(ctx, cam, w, h, b, spp, offset=0):
    n = hip.ansi_bytes(w, h)
    mem = DeviceBytes(n, offset)
    ctx.render_device_ansi(cam, hip.RowSet.whole(w, h), b, spp, mem.ptr, n)
    return mem.read(ctx, "full text")


def half_of_device_rgb8(ctx, rgb, offset=0, what=""):
    """trt_ansi_half_from_rgb8_device of a frame of bytes [rows, w, 3] uploaded at an odd address"""
    import torch
    rows, w, _ = rgb.shape
    src = torch.zeros(rgb.size + 1, dtype=torch.uint8, device="cuda:0")
    src[1:] = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1)).to("cuda:0")
    mem = DeviceBytes(hip.ansi_half_bytes(w, rows), offset)
    torch.cuda.synchronize()
    ctx.ansi_half_from_rgb8(src.data_ptr() + 1, w, rows, mem.ptr)
    return mem.read(ctx, what)


# ---- 1. any size, any alignment ----

SIZES = [(1, 1, 10), (1, 2, 3), (1, 5, 1), (2, 3, 10), (3, 2, 3), (4, 4, 1), (7, 5, 10), (33, 3, 3), (67, 13, 10)]


def test_the_widths_one_to_four_give_row_lengths_of_every_residue():
    assert {w for w, _, _ in SIZES} >= {1, 2, 3, 4} and {(CELL * w + END) % STORE for w in (1, 2, 3, 4)} == {0, 1, 2, 3}


@pytest.mark.parametrize("w,h,spp", SIZES, ids=[f"{w}x{h}_spp{s}" for w, h, s in SIZES])
def test_any_alignment_and_any_size(ctx, w, h, spp):
    """end bytes behind every cell (w = 1), row lengths 39 w + 5 of every residue modulo 4 (w = 1..4), odd and even row counts (an odd frame's
    last lower pixels are 000;000;000), a wave's 2304 bytes across several text rows, several waves (67 x 13: 18 333 bytes) -- at every residue
    of the output address modulo the store's four bytes: the emitter's bytes, and not a byte outside them"""
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[2]
    for offset in range(STORE):
        same_text(device_half(ctx, cam, w, h, 4, spp, offset, what=f"offset {offset}"), want, f"{w}x{h} spp {spp} at offset {offset}")


def span_edge_widths():
    """the widths at which the last byte of the first wave's span (of a text at an aligned address) lies in the last cell of text row 0, one cell
    before it, and in cell 0 of text row 1 -- from the words a wave stores, as the binding reads them from the layout header"""
    last = STORE * hip.ANSI_HALF_WAVE_WORDS - 1 - HOME  # byte of row 0's cells, were the row long enough
    col = last // CELL
    in_last, before_last, into_next = col + 1, col + 2, (last - END) // CELL
    assert CELL * in_last + END > last and 0 <= last - (CELL * into_next + END) < CELL
    return [in_last, before_last, into_next]


@pytest.mark.parametrize("h", [3, 4])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["in_the_last_cell", "one_cell_before", "one_cell_into_row_1"])
def test_rows_that_end_around_the_end_of_the_first_waves_span(ctx, which, h):
    w = span_edge_widths()[which]
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, 3)[2]
    for offset in range(STORE):
        same_text(device_half(ctx, cam, w, h, 4, 3, offset, what=f"offset {offset}"), want, f"{w}x{h} at offset {offset}")


# ---- 2. the frames of a batch start anywhere ----

def test_the_frames_of_a_batch_start_at_any_alignment(ctx):
    """four frames of 7 743 bytes (3 modulo 4) from offset 1: they start at residues 1, 0, 3 and 2.  The row count is odd: a lower pixel read
    from the scratch behind a frame's last row would show the next frame's top row"""
    w, h, indices = 66, 5, [7, 21, 33, 47]
    assert hip.ansi_half_bytes(w, h) == 7743 and [(1 + k * 7743) % STORE for k in range(4)] == [1, 0, 3, 2]
    ctx.set_scene(scene("demo"))
    cams = anim_cameras(indices, w, h)
    for spp in (10, 3):
        got = batch_half(ctx, cams, w, h, 4, spp, offset=1, what=f"batch of 4, spp {spp}")
        assert ctx.batch_info() == (4, 1)
        for k, index in enumerate(indices):
            want = oracle("demo", w, h, index, 4, spp)[2]
            assert want[-(CELL * w + END):].tobytes().count(b";48;2;000;000;000m") == w  # the odd frame's last lower pixels
            same_text(got[k], want, f"frame {k} of the batch, spp {spp}")


ONE = [(66, 5, 3), (2, 2, 1)]  # 7 743 bytes: the text ends mid-word; 89 bytes: less than a wave's span


@pytest.mark.parametrize("w,h,spp", ONE, ids=[f"{w}x{h}_spp{s}" for w, h, s in ONE])
def test_a_batch_of_one_is_the_single_frame_entry_at_any_alignment(ctx, w, h, spp):
    assert hip.ansi_half_bytes(w, h) % STORE != 0 and (hip.ansi_half_bytes(w, h) == 7743 or hip.ansi_half_bytes(w, h) == 89 < STORE * hip.ANSI_HALF_WAVE_WORDS)
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[2]
    for offset in range(STORE):
        single = device_half(ctx, cam, w, h, 4, spp, offset, what=f"single, offset {offset}")
        batch = batch_half(ctx, np.array([cam]), w, h, 4, spp, offset, what=f"batch of one, offset {offset}")
        assert ctx.batch_info() == (1, 1)
        same_text(batch[0], single, f"{w}x{h} spp {spp}: a batch of one against the single entry at offset {offset}")
        same_text(single, want, f"{w}x{h} spp {spp} at offset {offset}")


# ---- 3. every output kind on one context ----

def test_every_output_kind_interleaved_on_one_context():
    """doubles, bytes, text and half-block text; single frames and batches; host and device entries, in turn, twice round: a queue that a
    half-block frame leaves unready for the next kind (or the reverse), a scratch sized for another kind or a history entry left open would
    show in a frame or in the count of kernel times"""
    w, h, b, spp = 160, 48, 4, 3
    rows = hip.RowSet.whole(w, h)
    indices = [0, 19, 59]
    cams = anim_cameras(indices, w, h)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    px, rgb, half = ([oracle("synth64", w, h, i, b, spp)[k] for i in indices] for k in range(3))
    full = [full_text(r) for r in rgb]
    with hip.Context(0) as c:
        c.set_scene(scene("synth64"))
        calls = 0
        for turn in range(2):
            assert np.array_equal(bits(c.render_host(cams[0], rows, b, spp)), bits(px[0])), turn
            same_text(c.render_host_ansi_half(cams[1], rows, b, spp), half[1], f"render_host_ansi_half, turn {turn}")
            same_bytes(c.render_host_rgb8(cams[2], rows, b, spp), rgb[2], f"render_host_rgb8 after half-block text, turn {turn}")
            same_text(device_half(c, cams[2], w, h, b, spp, offset=turn + 1), half[2], f"render_device_ansi_half, turn {turn}")
            same_text(c.render_host_ansi(cams[0], rows, b, spp), full[0], f"render_host_ansi after half-block text, turn {turn}")
            got = batch_half(c, cams, w, h, b, spp, offset=3 - turn)
            assert c.batch_info() == (3, 1)
            for k in range(3):
                same_text(got[k], half[k], f"render_batch_ansi_half frame {k}, turn {turn}")
            frames = c.render_host_batch(cams, rows, b, spp)
            for k in range(3):
                assert np.array_equal(bits(frames[k]), bits(px[k])), (turn, k)
            got = c.render_host_batch_ansi_half(cams[::-1].copy(), rows, b, spp)
            for k in range(3):
                same_text(got[k], half[2 - k], f"render_host_batch_ansi_half frame {k}, turn {turn}")
            got = c.render_host_batch_rgb8(cams, rows, b, spp)
            for k in range(3):
                same_bytes(got[k], rgb[k], f"render_host_batch_rgb8 after a half-block batch, frame {k}, turn {turn}")
            got = c.render_host_batch_ansi(cams, rows, b, spp)
            for k in range(3):
                same_text(got[k], full[k], f"render_host_batch_ansi frame {k}, turn {turn}")
            same_text(device_full(c, cams[1], w, h, b, spp, offset=turn), full[1], f"render_device_ansi, turn {turn}")
            calls += 11
            assert c.launch_count() == calls
        times = c.kernel_times()
        assert len(times) == calls and all(t > 0 for t in times)
        render_ms, reduce_ms = c.render_kernel_times()
        assert len(render_ms) == calls and len(reduce_ms) == calls and all(t > 0 for t in render_ms) and all(t > 0 for t in reduce_ms)


# ---- 4. the instantiations ----

def _decoupled(c):
    c.set_compaction(1)
    return "synth64", lambda: c.render_variant()["decoupled"]


def _patches(c):
    c.set_path_patches(2)
    return "synth32", lambda: c.path_patches()[0] == 2 and c.render_variant()["workgroup_threads"] in (256, 1024)


def _image(c):
    c.set_scene_image(1)
    return "synth64", lambda: c.render_image()["in_device_memory"]


def _counting(c):
    c.enable_counters(True)
    return "synth64", lambda: True


def _reference(c):
    c.set_kernel(hip.Context.REFERENCE_ORDER)
    return "synth64", lambda: c.render_variant()["workgroup_threads"] == 256


@pytest.mark.parametrize("setup", [_decoupled, _patches, _image, _counting, _reference], ids=lambda f: f.__name__.strip("_"))
def test_the_half_block_text_through_every_instantiation(ctx, setup):
    w, h, b, spp, index = 96, 32, 4, 3, 19
    kind, ran = setup(ctx)
    ctx.set_scene(scene(kind))
    cam = anim_cameras([index], w, h)[0]
    _, rgb, want, counts = oracle(kind, w, h, index, b, spp)
    same_text(device_half(ctx, cam, w, h, b, spp, offset=1, what=setup.__name__), want, setup.__name__ + ", device entry")
    assert ran(), setup.__name__
    if setup is _counting:
        assert ctx.read_counters() == counts
    same_text(ctx.render_host_ansi_half(cam, hip.RowSet.whole(w, h), b, spp), want, setup.__name__ + ", host entry")
    rows = hip.RowSet.shard(w, h, 1, 3, 4)
    owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(owned_rows(rows))]
    assert 0 < len(owned) < h
    # a shard's rows pair up in local order: local rows 2 i and 2 i + 1
    same_text(device_half(ctx, cam, w, h, b, spp, offset=3, rows=rows), half_text(np.ascontiguousarray(rgb[owned])), setup.__name__ + ", a shard")


# ---- 5. filled scratch and filled output ----

def test_a_filled_scratch_and_a_filled_output_leave_the_emitters_text(ctx):
    """trt_set_scratch_fill: the launch's samples and exactly its text bytes are 0xFF before the launch -- a NaN in every double, which the cast
    turns into 0 and the text into 000 -- so a sample the render kernel drops prints 000 where the oracle does not, and a text byte the pass
    skips stays 0xFF (the glyph's bytes are E2 96 80: no byte of a text is 0xFF); the bytes around the text keep their 0xA5"""
    ctx.set_scratch_fill(True)
    ctx.set_scene(scene("demo"))
    for w, h, spp in ((67, 13, 10), (7, 5, 10)):
        cam = anim_cameras([7], w, h)[0]
        _, rgb, want, _ = oracle("demo", w, h, 7, 4, spp)
        assert (rgb != 0).any() and not (want == 0xFF).any()
        for offset in (0, 3):
            same_text(device_half(ctx, cam, w, h, 4, spp, offset, what="filled"), want, f"filled, {w}x{h} at offset {offset}")
        same_text(ctx.render_host_ansi_half(cam, hip.RowSet.whole(w, h), 4, spp), want, f"filled, {w}x{h}, host entry")
    w, h, indices = 7, 5, [7, 21, 33]
    got = batch_half(ctx, anim_cameras(indices, w, h), w, h, 4, 10, offset=2, what="filled batch")
    for k, index in enumerate(indices):
        want = oracle("demo", w, h, index, 4, 10)[2]
        assert not (want == 0xFF).any()
        same_text(got[k], want, f"filled batch, frame {k}")
    ctx.set_kernel(hip.Context.REFERENCE_ORDER)
    same_text(device_half(ctx, anim_cameras([7], 7, 5)[0], 7, 5, 4, 10, offset=1, what="filled, reference-order"), oracle("demo", 7, 5, 7, 4, 10)[2],
              "filled, reference-order kernel")


# ---- 6. the formatting alone ----

def test_ansi_half_from_rgb8_formats_every_digit_triple_at_every_alignment(ctx):
    """a 16 x 16 image with r = i, g = 255 - i, b = 7 i mod 256: every value of every channel, in upper and in lower pixels; a 5 x 3 image (an
    odd frame) at offsets 0..3, into text bytes that held 0xA5"""
    i = np.arange(256)
    image = np.stack([i, 255 - i, (7 * i) & 255], axis=1).astype(np.uint8).reshape(16, 16, 3)
    for ch in range(3):
        assert len(set(image[..., ch].ravel())) == 256
    same_text(half_of_device_rgb8(ctx, image, offset=1, what="16 x 16"), half_text(image), "16 x 16, every digit triple")
    flipped = np.ascontiguousarray(image[::-1])  # the values the upper pixels took, in lower pixels
    same_text(half_of_device_rgb8(ctx, flipped, offset=3, what="16 x 16 flipped"), half_text(flipped), "16 x 16 flipped")
    small = np.random.default_rng(5).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    for offset in range(STORE):
        same_text(half_of_device_rgb8(ctx, small, offset, what=f"5 x 3 at offset {offset}"), half_text(small), f"5 x 3 at offset {offset}")
    lib, p = hip.lib(), C.c_void_p(DeviceBytes(64).ptr)
    assert lib.trt_ansi_half_from_rgb8_device(None, p, 1, 1, p) == ARGUMENT and lib.trt_ansi_half_from_rgb8_device(ctx._h, None, 1, 1, p) == ARGUMENT
    assert lib.trt_ansi_half_from_rgb8_device(ctx._h, p, 1, 1, None) == ARGUMENT
    assert lib.trt_ansi_half_from_rgb8_device(ctx._h, p, 0, 1, p) == ARGUMENT and lib.trt_ansi_half_from_rgb8_device(ctx._h, p, 1, -1, p) == ARGUMENT


# ---- 7. the delta entries are undisturbed ----

def test_a_half_block_frame_leaves_the_delta_entries_shown_frame_alone():
    w, h, b, spp = 33, 6, 4, 3
    rows = hip.RowSet.whole(w, h)
    cams = anim_cameras([7, 33], w, h)
    with hip.Context(0) as c:
        c.set_scene(scene("demo"))
        key = c.render_host_ansi_delta(cams[0], rows, b, spp)
        assert key.size == hip.ansi_bytes(w, h)  # a keyframe
        same_text(c.render_host_ansi_half(cams[1], rows, b, spp), oracle("demo", w, h, 33, b, spp)[2], "the half-block frame of another camera")
        mem = DeviceBytes(hip.ansi_half_bytes(w, h), 1)
        c.render_device_ansi_half(cams[1], rows, b, spp, mem.ptr, mem.n)
        same_text(mem.read(c), oracle("demo", w, h, 33, b, spp)[2], "the device entry")
        assert c.render_host_ansi_delta(cams[0], rows, b, spp).size == 0, "the shown frame changed under a half-block frame"


# ---- 8. errors ----

def test_refusals_enqueue_nothing_and_leave_the_context_rendering(ctx):
    import torch
    lib = hip.lib()
    w, h, b, spp = 33, 3, 4, 3
    rows, bad_rows = hip.RowSet.whole(w, h), hip.RowSet(0, h, h, 0, 1)
    cams = anim_cameras([7, 21], w, h)
    cam = hip.camera_struct(cams[0])
    n = hip.ansi_half_bytes(w, h)
    mem = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    text = np.full(2 * n, 0xA5, dtype=np.uint8)
    torch.cuda.synchronize()
    p, hp, cp, r = C.c_void_p(mem.data_ptr()), C.c_void_p(text.ctypes.data), C.c_void_p(cams.ctypes.data), C.byref(rows)
    single = lambda c, camera=C.byref(cam), rs=r, bl=b, out=p, cap=n: lib.trt_render_device_ansi_half(c, camera, rs, bl, spp, out, cap)
    batch = lambda c, cameras=cp, k=2, rs=r, bl=b, out=p, cap=2 * n: lib.trt_render_device_batch_ansi_half(c, cameras, k, rs, bl, spp, out, cap)
    hsingle = lambda c, camera=C.byref(cam), rs=r, bl=b, out=hp: lib.trt_render_host_ansi_half(c, camera, rs, bl, spp, out)
    hbatch = lambda c, cameras=cp, k=2, rs=r, bl=b, out=hp: lib.trt_render_host_batch_ansi_half(c, cameras, k, rs, bl, spp, out)
    # the entries each one mirrors: a refusal returns the code the _ansi entry returns
    m_single = lambda c, camera=C.byref(cam), rs=r, bl=b, out=p, cap=n: lib.trt_render_device_ansi(c, camera, rs, bl, spp, out, cap)
    m_batch = lambda c, cameras=cp, k=2, rs=r, bl=b, out=p, cap=2 * n: lib.trt_render_device_batch_ansi(c, cameras, k, rs, bl, spp, out, cap)
    m_hsingle = lambda c, camera=C.byref(cam), rs=r, bl=b, out=hp: lib.trt_render_host_ansi(c, camera, rs, bl, spp, out)
    m_hbatch = lambda c, cameras=cp, k=2, rs=r, bl=b, out=hp: lib.trt_render_host_batch_ansi(c, cameras, k, rs, bl, spp, out)
    pairs = ((single, m_single), (batch, m_batch), (hsingle, m_hsingle), (hbatch, m_hbatch))
    with hip.Context(0) as empty:
        for entry, mirror in pairs:
            assert entry(empty._h) == mirror(empty._h) == NO_SCENE
    ctx.set_scene(scene("demo"))
    h_ = ctx._h
    other = cams.copy()
    other[1, 13] *= 2
    for entry, mirror in pairs:
        refusals = [dict(c=None), dict(c=h_, out=None), dict(c=h_, rs=C.byref(bad_rows)), dict(c=h_, rs=None), dict(c=h_, bl=0)]
        if entry in (single, hsingle):
            refusals += [dict(c=h_, camera=None)]
        else:
            refusals += [dict(c=h_, cameras=None), dict(c=h_, k=0), dict(c=h_, k=9), dict(c=h_, cameras=C.c_void_p(other.ctypes.data))]
        for kw in refusals:
            assert entry(**kw) == mirror(**kw) == ARGUMENT, sorted(kw)
    assert single(h_, cap=n - 1) == CAPACITY and batch(h_, cap=2 * n - 1) == CAPACITY
    ctx.synchronize()
    assert (mem.cpu().numpy() == 0xA5).all(), "a refused device entry wrote to the caller's buffer"
    assert single(h_, cap=n) == 0 and batch(h_, cap=2 * n) == 0  # to the byte
    ctx.synchronize()
    assert (text == 0xA5).all(), "a refused host entry wrote to the caller's buffer"
    got = mem.cpu().numpy().reshape(2, n)
    for k, index in enumerate((7, 21)):
        same_text(got[k], oracle("demo", w, h, index, 4, spp)[2], f"the good call after the refusals, frame {k}")
    same_text(ctx.render_host_batch_ansi_half(cams, rows, b, spp)[1], oracle("demo", w, h, 21, 4, spp)[2], "the host batch after the refusals")
    same_text(ctx.render_host_ansi_half(cams[0], rows, b, spp), oracle("demo", w, h, 7, 4, spp)[2], "the host entry after the refusals")


# ---- 9. the drop-in entry and the demo ----

def test_the_drop_in_entry_gives_the_device_entrys_text(ctx):
    """demo_160x48_b4, the reference's golden scene: 149 886 bytes through trt_render_frame_ansi_half on a fresh default context, through the
    device entry and through trt_ansi_half_from_rgb8_device of the RGB8 entry's bytes, all of them the emitter's text of the oracle's bytes"""
    name = "demo_160x48_b4"
    case = next(c for c in T.golden_cases() if c["name"] == name)
    w, h, b, spp = case["width"], case["height"], case["bounce_limit"], case["rays_per_pixel"]
    assert hip.ansi_half_bytes(w, h) == 149886
    sc = T.golden_scene(case)
    px, _ = T.oracle_render(sc, w, h, b, spp)
    assert T.fnv(px) == case["fb_fnv"]
    want = half_text(T.oracle_rgb8(px))
    ctx.set_scene(sc)
    device = device_half(ctx, sc.camera, w, h, b, spp, offset=1, what=name)
    same_text(device, want, name + " through trt_render_device_ansi_half")
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    same_text(hip.render_frame_ansi_half(sc, w, h, b, spp), device, name + " through trt_render_frame_ansi_half")
    same_text(hip.render_frame_ansi_half(sc, w, h, b, spp), device, name + " through trt_render_frame_ansi_half, again")
    hip._check(hip.lib().trt_shutdown())


def rgb_of_full_text(text, w, h):
    """the bytes a full text (trt_ansi.h: 25-byte cells, digits at 7, 11, 15) shows: uint8 [h, w, 3]"""
    a = np.frombuffer(text, dtype=np.uint8)[HOME:HOME + (25 * w + 1) * h].reshape(h, 25 * w + 1)[:, :25 * w].reshape(h, w, 25).astype(np.int32) - ord("0")
    return np.stack([100 * a[..., at] + 10 * a[..., at + 1] + a[..., at + 2] for at in (7, 11, 15)], axis=-1).astype(np.uint8)


def test_demo_program_writes_the_devices_half_block_text(tmp_path):
    """examples/trt_demo --half: trt_render_frame_ansi_half into a buffer of trt_ansi_half_bytes, one fwrite, no emitter -- three texts of
    149 886 bytes and the fps lines, the first of them the host emitter's half-block text of the frame --rgb8 wrote"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    n = hip.ansi_half_bytes(160, 48)
    assert n == 149886
    # --step: frame k at orbit time 0.04 k in both runs (the wall clock's times differ from run to run)
    half = subprocess.run([exe, str(sky), "3", "160", "48", "--half", "--step=0.04"], capture_output=True, timeout=120)
    assert half.returncode == 0, half.stderr[-500:]
    assert b"3 frames 160x48" in half.stderr and b"as half-block text" in half.stderr
    assert half.stdout.count(b"\xe2\x96\x80") == 3 * 160 * 24
    assert len(half.stdout) >= 3 * n
    rgb8 = subprocess.run([exe, str(sky), "3", "160", "48", "--rgb8", "--step=0.04"], capture_output=True, timeout=120)
    assert rgb8.returncode == 0, rgb8.stderr[-500:]
    first = rgb_of_full_text(rgb8.stdout[:hip.ansi_bytes(160, 48)], 160, 48)
    assert len(np.unique(first.reshape(-1, 3), axis=0)) > 12, "a frame of one colour"
    assert half.stdout[:n] == half_text(first).tobytes()
