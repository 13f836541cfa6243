"""The ordered mean's doubles pass (reduce_samples_kernel, csrc/trt_common.hpp): a lane owns a group of consecutive values
(csrc/trt_mean_lanes.h), fetches a block of DEEP samples of them with 16-byte loads before the first add and stores the group at once.
Frame sizes either side of the lane map's edges, sample counts either side of the block, frames and buffers that are 8-byte aligned
and no more, batches, a filled scratch and every instantiation of the render kernel in front of the pass.  The expected frames never
come from the library: they are T.oracle_render's doubles, compared as bits."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import support as T
from support import anim_cameras
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

gpu = pytest.mark.gpu
CSRC = os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")
DEEP = int(re.search(r"^#define TRT_REDUCE_DEEP (\d+)", open(os.path.join(CSRC, "trt_common.hpp")).read(), re.M).group(1))
GUARD = 64  # bytes of PATTERN either side of every device buffer
PATTERN = 0x5A5AC3C35A5AC3C3


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


@functools.lru_cache(maxsize=None)
def oracle(kind, w, h, index, b, spp):
    """(the oracle's double frame, (path rays, shadow rays)) -- computed once, never written to"""
    px, st = T.oracle_render(scene(kind).with_camera(anim_cameras([index], w, h)[0]), w, h, b, spp)
    px.flags.writeable = False
    return px, (st.path_rays, st.shadow_rays)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wrong = got != want
    assert not wrong.any(), f"{what}: {int(wrong.sum())} of {wrong.size} values differ from the oracle's, the first at {int(np.argmax(wrong.reshape(-1)))}"


class DeviceDoubles:
    """n doubles of device memory that start `offset` (0 or 8) bytes behind a 16-byte-aligned address, GUARD bytes of PATTERN in front
    and behind"""

    def __init__(self, n, offset=0):
        import torch
        assert offset in (0, 8) and GUARD % 16 == 0
        self.n, self.start = n, (GUARD + offset) // 8
        self.buf = torch.full((GUARD // 8 + 1 + n + GUARD // 8,), PATTERN, dtype=torch.int64, device="cuda:0")
        assert self.buf.data_ptr() % 16 == 0
        torch.cuda.synchronize()  # the fill is on torch's stream, the render on the context's

    @property
    def ptr(self):
        return self.buf.data_ptr() + 8 * self.start

    def read(self, ctx, what=""):
        """the n doubles, once every word outside them has been seen unchanged"""
        ctx.synchronize()
        host = self.buf.cpu().numpy().view(np.uint64)
        outside = np.concatenate([host[:self.start], host[self.start + self.n:]])
        assert outside.size >= 2 * GUARD // 8 and (outside == PATTERN).all(), f"{what}: {int((outside != PATTERN).sum())} words outside the frame were written"
        return host[self.start:self.start + self.n].copy().view(np.float64)


def device_frame(ctx, cam, w, h, b, spp, offset=0, rows=None, what=""):
    rows = rows or hip.RowSet.whole(w, h)
    n = hip.lib().trt_rowset_rows(C.byref(rows)) * w * 3
    mem = DeviceDoubles(n, offset)
    assert mem.ptr % 16 == offset
    ctx.render_device(cam, rows, b, spp, mem.ptr, n * 8)
    return mem.read(ctx, what).reshape(-1, w, 3)


def device_batch(ctx, cams, w, h, b, spp, offset=0, what=""):
    n = len(cams) * h * w * 3
    mem = DeviceDoubles(n, offset)
    ctx.render_device_batch(cams, hip.RowSet.whole(w, h), b, spp, mem.ptr, n * 8)
    return mem.read(ctx, what).reshape(len(cams), h, w, 3)


# ---- 1. the lane map on the host ----

@pytest.mark.parametrize("group", [None, 1, 4], ids=["as_shipped", "group1", "group4"])
def test_every_value_has_exactly_one_lane(group):
    """csrc/trt_mean_lanes.h compiled for the host in tests/mean_lanes_check.c: frames of 1 .. 399 values, as the library ships the map and
    at the other groups it can be built with"""
    build = os.path.join(T.ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, f"mean_lanes_check_{group or 'shipped'}")
    flags = [f"-DTRT_MEAN_GROUP={group}"] if group else []
    made = subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags + ["-o", exe, os.path.join(T.ROOT, "tests", "mean_lanes_check.c")],
                          capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and "mean_lanes_check: ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]


# ---- 2. sizes that straddle the lane map, depths that straddle the block ----

SIZES = [(1, 1), (7, 5), (21, 2), (43, 1), (64, 1), (67, 13)]  # values: 3 (a tail only), 105, 126, 129 (a second wave: a pair and a tail), 192, 2613


@gpu
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes_either_side_of_the_lane_map(ctx, w, h):
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    for spp in (10, 3):
        want = oracle("demo", w, h, 7, 4, spp)[0]
        same_bits(device_frame(ctx, cam, w, h, 4, spp, what=f"{w}x{h} spp {spp}"), want, f"{w}x{h} spp {spp}")


DEPTHS = sorted({1, 2, DEEP - 1, DEEP, DEEP + 1, 2 * DEEP, 2 * DEEP + 1, 10} - {0})


@gpu
@pytest.mark.parametrize("w,h", [(7, 5), (43, 1)], ids=["7x5", "43x1"])
@pytest.mark.parametrize("spp", DEPTHS)
def test_sample_counts_either_side_of_the_block(ctx, w, h, spp):
    """no block, a block to the sample, a block and a remainder, two blocks, two and a remainder"""
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    same_bits(device_frame(ctx, cam, w, h, 4, spp, what=f"spp {spp}"), oracle("demo", w, h, 7, 4, spp)[0], f"{w}x{h} spp {spp}")


# ---- 3. alignment and guards ----

@gpu
@pytest.mark.parametrize("w,h,spp", [(7, 5, 10), (7, 5, 3), (67, 13, 10), (64, 1, 3), (1, 1, 10)], ids=lambda v: str(v))
def test_a_buffer_that_is_8_byte_aligned_and_no_more(ctx, w, h, spp):
    """the caller's buffer 0 and 8 bytes behind a 16-byte-aligned address: the oracle's frame, not a word outside it, and the host entry's
    frame is the same"""
    ctx.set_scene(scene("demo"))
    cam = anim_cameras([7], w, h)[0]
    want = oracle("demo", w, h, 7, 4, spp)[0]
    for offset in (0, 8):
        same_bits(device_frame(ctx, cam, w, h, 4, spp, offset, what=f"offset {offset}"), want, f"{w}x{h} spp {spp} at offset {offset}")
    same_bits(ctx.render_host(cam, hip.RowSet.whole(w, h), 4, spp), want, f"{w}x{h} spp {spp}, host entry")


# ---- 4. batches ----

@gpu
@pytest.mark.parametrize("spp", [3, 10])
def test_the_frames_of_a_batch_start_at_odd_multiples_of_8_bytes(ctx, spp):
    """three frames of 105 values: frame 1 starts an odd number of doubles behind frame 0 in the output (and, spp 3, in the scratch),
    frame 2 an even number -- from a buffer at offset 0 and at offset 8, so each frame is seen at both alignments"""
    w, h, indices = 7, 5, [7, 21, 33]
    assert (w * h * 3) % 2 == 1
    ctx.set_scene(scene("demo"))
    cams = anim_cameras(indices, w, h)
    for offset in (0, 8):
        got = device_batch(ctx, cams, w, h, 4, spp, offset, what=f"batch of 3, spp {spp}, offset {offset}")
        assert ctx.batch_info() == (3, 1)
        for k, index in enumerate(indices):
            same_bits(got[k], oracle("demo", w, h, index, 4, spp)[0], f"frame {k} of the batch, spp {spp}, offset {offset}")


# ---- 5. a filled scratch ----

@gpu
def test_a_filled_scratch_and_a_filled_output_leave_the_oracles_frame(ctx):
    """trt_set_scratch_fill: the launch's samples and its pixels are NaN before the launch, so a sample the pass does not add (or adds
    from the wrong place) and a value it does not store show"""
    ctx.set_scratch_fill(True)
    ctx.set_scene(scene("demo"))
    for w, h, spp in ((67, 13, 10), (7, 5, 3), (7, 5, DEEP + 1)):
        cam = anim_cameras([7], w, h)[0]
        want = oracle("demo", w, h, 7, 4, spp)[0]
        assert not np.isnan(want).any()
        for offset in (0, 8):
            same_bits(device_frame(ctx, cam, w, h, 4, spp, offset, what="filled"), want, f"filled, {w}x{h} spp {spp} at offset {offset}")
        same_bits(ctx.render_host(cam, hip.RowSet.whole(w, h), 4, spp), want, f"filled, {w}x{h} spp {spp}, host entry")
    w, h, indices = 7, 5, [7, 21, 33]
    got = device_batch(ctx, anim_cameras(indices, w, h), w, h, 4, 3, offset=8, what="filled batch")
    for k, index in enumerate(indices):
        same_bits(got[k], oracle("demo", w, h, index, 4, 3)[0], f"filled batch, frame {k}")


# ---- 6. the instantiations ----

def _decoupled(c):
    c.set_compaction(1)
    return "synth64", lambda: c.render_variant()["decoupled"]


def _plain(c):
    c.set_compaction(0)
    return "synth64", lambda: not c.render_variant()["decoupled"]


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


@gpu
@pytest.mark.parametrize("setup", [_decoupled, _plain, _patches, _image, _counting, _reference], ids=lambda f: f.__name__.strip("_"))
def test_the_doubles_path_through_every_instantiation(ctx, setup):
    w, h, b, spp, index = 96, 32, 4, 3, 19
    kind, ran = setup(ctx)
    ctx.set_scene(scene(kind))
    cam = anim_cameras([index], w, h)[0]
    want, counts = oracle(kind, w, h, index, b, spp)
    same_bits(device_frame(ctx, cam, w, h, b, spp, offset=8, what=setup.__name__), want, setup.__name__ + ", device entry")
    assert ran(), setup.__name__
    if setup is _counting:
        assert ctx.read_counters() == counts
    same_bits(ctx.render_host(cam, hip.RowSet.whole(w, h), b, spp), want, setup.__name__ + ", host entry")
    rows = hip.RowSet.shard(w, h, 1, 3, 4)
    owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(hip.lib().trt_rowset_rows(C.byref(rows)))]
    same_bits(device_frame(ctx, cam, w, h, b, spp, offset=8, rows=rows), want[owned], setup.__name__ + ", a shard")
