"""The frame as a DEC sixel image written on the device (trt_sixel_from_rgb8_device, trt_render_device_sixel, trt_render_host_sixel,
trt_render_frame_sixel): three kernels in stream order behind the RGB8 form of the ordered mean -- a 240-bit colour mask per band of six
rows, one workgroup's scan of the bands' colour counts, and a thread per four adjacent columns that walks its band's mask and stores an
aligned 32-bit word per colour (csrc/trt_sixel.h, trt_sixel.hpp).  The expected bytes never come from the library's device route: they are
the sequential host emitter's (host.emitter_sixel_rgb8, which tests/test_sixel_layout.py holds against a formatter with a palette search of
its own, a literal and a structural reader) of the bytes given, or of T.oracle_rgb8 -- the CPU checker's (int)(c*255) -- of the oracle's
double frame, and the structural reader (tests/sixel_support.py) reads every rendered text back to the oracle's frame of palette indices."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import sixel_support as X
import support as T
from support import GUARD, STORE, anim_cameras
from terminalraytracer_amd import hip, host
from terminalraytracer_amd import scenes as S

pytestmark = pytest.mark.gpu
ARGUMENT, NO_SCENE, CAPACITY = -2, -3, -4
SENTINEL = 0x1111111111111111
SCAN_BLOCK = hip._header_constant("trt_sixel.h", "TRT_SIXEL_SCAN_BLOCK")  # bands the offsets kernel scans per turn
TILE = hip._header_constant("trt_sixel.h", "TRT_SIXEL_BLOCK")            # slots, four columns each, of a write workgroup
# (width, rows) of tests/test_sixel_layout.py: every T, colour rows shorter than a word, short and whole bands; 63, 64, 65, 257 wide
SIZES = [(w, h) for w in (1, 2, 3, 4, 5) for h in (1, 5, 6, 7, 13)] + [(63, 7), (64, 6), (65, 13), (257, 5), (257, 13)]
RENDERED = [(13, 5, 2, 3), (41, 25, 2, 3), (160, 48, 4, 10)]  # (width, rows, bounce limit, rays per pixel)
INDEX = 7        # the camera of the orbit every single frame is rendered from


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield
    if "ctx" in request.fixturenames:
        request.getfixturevalue("ctx").set_kernel(hip.Context.PRODUCTION)


@functools.lru_cache(maxsize=None)
def scene():
    return S.demo_scene(T.sky("synth"), anim_cameras([0], 160, 48)[0])


def sixel_text(rgb):
    """the host emitter's image of a frame of bytes [rows, w, 3]"""
    rows, w, _ = rgb.shape
    text = host.emitter_sixel_rgb8(rgb)
    assert X.FIXED < text.size <= X.capacity(w, rows) == hip.sixel_capacity(w, rows)
    return text


@functools.lru_cache(maxsize=None)
def oracle(w, h, index, b, spp):
    """(the oracle's bytes by the checker's cast, the emitter's image of those) -- computed once, never written to"""
    px, _ = T.oracle_render(scene().with_camera(anim_cameras([index], w, h)[0]), w, h, b, spp)
    rgb = T.oracle_rgb8(px)
    text = sixel_text(rgb)
    rgb.flags.writeable = text.flags.writeable = False
    return rgb, text


class DeviceText:
    """`capacity` bytes of device memory that start `offset` bytes behind a 4-aligned address and hold `fill`, GUARD bytes of 0xA5 in front
    and behind; and the length's uint64 between two more that hold a sentinel"""

    def __init__(self, capacity, offset=0, fill=0xA5):
        import torch
        self.capacity, self.start, self.fill = capacity, GUARD + offset, fill
        self.buf = torch.full((GUARD + STORE + capacity + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.buf[self.start:self.start + capacity] = fill
        self.lengths = torch.full((3,), SENTINEL, dtype=torch.int64, device="cuda:0")
        assert self.buf.data_ptr() % STORE == 0 and GUARD % STORE == 0 and self.lengths.data_ptr() % 8 == 0
        torch.cuda.synchronize()  # the fills are on torch's stream, the kernels on the context's

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    @property
    def bytes_ptr(self):
        return self.lengths.data_ptr() + 8

    def read(self, ctx, what=""):
        """the text, once its length is seen between its sentinels and every byte outside the text has been seen unchanged"""
        ctx.synchronize()
        lengths = [int(k) for k in self.lengths.cpu()]
        assert lengths[0] == SENTINEL and lengths[2] == SENTINEL, f"{what}: a store beside the length"
        n = lengths[1]
        assert X.FIXED < n <= self.capacity, f"{what}: a length of {n} in a room of {self.capacity}"
        got = self.buf.cpu().numpy()
        assert (got[:self.start] == 0xA5).all() and (got[self.start + self.capacity:] == 0xA5).all(), f"{what}: bytes outside the buffer were written"
        behind = got[self.start + n:self.start + self.capacity]
        assert (behind == self.fill).all(), f"{what}: {int((behind != self.fill).sum())} bytes at or behind the length {n} were written"
        return got[self.start:self.start + n].copy()

    def untouched(self, ctx):
        ctx.synchronize()
        got = self.buf.cpu().numpy()
        inside = got[self.start:self.start + self.capacity]
        return bool((inside == self.fill).all()) and int((got == 0xA5).sum()) >= got.size - self.capacity and [int(k) for k in self.lengths.cpu()] == [SENTINEL] * 3


def same_text(got, want, what, index=None):
    """byte for byte the emitter's, the length too; and, where the frame of indices is given, what the structural reader reads"""
    T.same_text(got, want, what)
    if index is not None:
        assert np.array_equal(X.read(np.asarray(got).tobytes()), index), what + ": the structural reader reads another frame"


def upload(rgb):
    """the frame one byte behind an aligned address"""
    import torch
    src = torch.zeros(rgb.size + 1, dtype=torch.uint8, device="cuda:0")
    src[1:] = torch.from_numpy(np.ascontiguousarray(rgb).reshape(-1)).to("cuda:0")
    torch.cuda.synchronize()
    return src


def from_rgb8_everywhere(ctx, rgb, what):
    """trt_sixel_from_rgb8_device at the offsets 0..3, each into a buffer of 0xA5 and into one of 0x5A: the emitter's text, its length, nothing
    at or behind it -- and the two runs equal, so no byte was left as it was"""
    rows, w, _ = rgb.shape
    want, src, room = sixel_text(rgb), upload(rgb), hip.sixel_capacity(w, rows)
    index = X.search(rgb)
    for offset in range(STORE):
        texts = []
        for fill in (0xA5, 0x5A):
            mem = DeviceText(room, offset, fill)
            ctx.sixel_from_rgb8(src.data_ptr() + 1, w, rows, mem.ptr, room, mem.bytes_ptr)
            texts.append(mem.read(ctx, f"{what} at offset {offset}"))
        same_text(texts[0], want, f"{what} at offset {offset}", index if offset == 0 else None)
        assert np.array_equal(texts[0], texts[1]), f"{what} at offset {offset}: the text depends on what the buffer held"


# ---- 1. the formatting alone: every T, short rows, short bands, the tile's and the scan's edges, at any alignment ----

def _image(w, h, colours=None):
    rng = np.random.default_rng(1000 * w + h)
    if colours is None:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return rng.integers(0, 256, (colours, 3), dtype=np.uint8)[rng.integers(0, colours, (h, w))]


@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_from_rgb8_formats_random_bytes_and_few_colours_at_every_alignment(ctx, w, h):
    from_rgb8_everywhere(ctx, _image(w, h), f"{w}x{h} random")
    from_rgb8_everywhere(ctx, _image(w, h, 3), f"{w}x{h} three colours")


def test_from_rgb8_one_colour_and_every_colour(ctx):
    from_rgb8_everywhere(ctx, np.full((13, 5, 3), (255, 0, 9), dtype=np.uint8), "one colour")
    every = X.every_colour_image()
    assert sixel_text(every).size == hip.sixel_capacity(40, 6) == 15872  # the length is the capacity: not a byte to spare
    from_rgb8_everywhere(ctx, every, "every colour once")


def test_from_rgb8_more_bands_than_the_scan_takes_in_a_turn(ctx):
    """a frame one pixel wide whose bands number two more than the offsets kernel's workgroup scans per turn: the running total crosses a turn"""
    rows = 6 * SCAN_BLOCK + 7
    assert (rows + 5) // 6 == SCAN_BLOCK + 2 and (SCAN_BLOCK != 1024 or rows == 6151)
    from_rgb8_everywhere(ctx, _image(1, rows, 7), f"1x{rows}")


def test_from_rgb8_a_row_wider_than_a_tile_of_columns(ctx):
    w = 4 * TILE + 1
    assert X.row_bytes(w) // 4 > TILE and (TILE != 256 or w == 1025)
    from_rgb8_everywhere(ctx, _image(w, 7, 40), f"{w}x7")


def test_from_rgb8_bands_that_alternate_between_one_colour_and_all(ctx):
    image = np.empty((30, 40, 3), dtype=np.uint8)
    image[:] = (255, 0, 9)
    for band in (1, 3):
        image[6 * band:6 * band + 6] = X.every_colour_image()
    assert X.colours_per_band(X.search(image)) == [1, 240, 1, 240, 1]
    from_rgb8_everywhere(ctx, image, "alternating bands")


def test_from_rgb8_refuses_before_it_writes(ctx):
    mem = DeviceText(hip.sixel_capacity(5, 7))
    lib, p, n, room = hip.lib(), C.c_void_p(mem.ptr), C.c_void_p(mem.bytes_ptr), hip.sixel_capacity(5, 7)
    call = lib.trt_sixel_from_rgb8_device
    assert call(None, p, 5, 7, p, room, n) == ARGUMENT and call(ctx._h, None, 5, 7, p, room, n) == ARGUMENT
    assert call(ctx._h, p, 5, 7, None, room, n) == ARGUMENT and call(ctx._h, p, 5, 7, p, room, None) == ARGUMENT
    assert call(ctx._h, p, 0, 7, p, room, n) == ARGUMENT and call(ctx._h, p, 5, -1, p, room, n) == ARGUMENT
    assert call(ctx._h, p, 100000, 1, p, 1 << 40, n) == ARGUMENT and call(ctx._h, p, 1, 100000, p, 1 << 40, n) == ARGUMENT
    assert call(ctx._h, p, 5, 7, p, room - 1, n) == CAPACITY and call(ctx._h, p, 5, 7, p, 0, n) == CAPACITY
    assert mem.untouched(ctx)


# ---- 2. rendered frames: both kernels, a shard, the host forms ----

def device_sixel(ctx, cam, w, h, b, spp, offset=0, rows=None, what="", fill=0xA5):
    rows = rows or hip.RowSet.whole(w, h)
    room = hip.sixel_capacity(w, hip.lib().trt_rowset_rows(C.byref(rows)))
    mem = DeviceText(room, offset, fill)
    ctx.render_device_sixel(cam, rows, b, spp, mem.ptr, room, mem.bytes_ptr)
    return mem.read(ctx, what)


@pytest.mark.parametrize("kernel", [hip.Context.PRODUCTION, hip.Context.REFERENCE_ORDER], ids=["production", "reference-order"])
@pytest.mark.parametrize("w,h,b,spp", RENDERED, ids=[f"{w}x{h}" for w, h, _, _ in RENDERED])
def test_rendered_frames_on_the_device_and_into_host_memory(ctx, w, h, b, spp, kernel):
    ctx.set_kernel(kernel)
    ctx.set_scene(scene())
    cam = anim_cameras([INDEX], w, h)[0]
    rgb, want = oracle(w, h, INDEX, b, spp)
    index = X.search(rgb)
    for offset in range(STORE):
        got = device_sixel(ctx, cam, w, h, b, spp, offset, what=f"offset {offset}", fill=0x5A if offset & 1 else 0xA5)
        same_text(got, want, f"{w}x{h} at offset {offset}", index if offset == 0 else None)
    same_text(ctx.render_host_sixel(cam, hip.RowSet.whole(w, h), b, spp), want, "render_host_sixel", index)


def test_the_shards_of_two_ranks_are_of_their_owned_rows_in_local_order(ctx):
    w, h, b, spp = 160, 48, 4, 10
    ctx.set_scene(scene())
    cam = anim_cameras([INDEX], w, h)[0]
    seen = []
    for rank in (0, 1):
        rows = hip.RowSet.shard(w, h, rank, 2, 5)  # tiles of five rows: the owned rows' bands straddle the tiles
        owned = [hip.lib().trt_rowset_frame_row(C.byref(rows), i) for i in range(hip.lib().trt_rowset_rows(C.byref(rows)))]
        assert 0 < len(owned) < h and owned[:6] == [10 * k + 5 * rank + j for k in (0, 1) for j in range(5)][:6]
        part = np.ascontiguousarray(oracle(w, h, INDEX, b, spp)[0][owned])
        got = device_sixel(ctx, cam, w, h, b, spp, offset=1 + rank, rows=rows, what=f"rank {rank}")
        same_text(got, sixel_text(part), f"the shard of rank {rank}", X.search(part))
        assert b'"1;1;00160;%05d#016' % len(owned) in got.tobytes()[:40]
        same_text(ctx.render_host_sixel(cam, rows, b, spp), sixel_text(part), f"the host form of rank {rank}'s shard")
        seen += owned
    assert sorted(seen) == list(range(h))


def test_the_drop_in_entry_on_the_default_context():
    w, h, b, spp = 160, 48, 4, 10
    rgb, want = oracle(w, h, 21, b, spp)
    hip._check(hip.lib().trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    there = scene().with_camera(anim_cameras([21], w, h)[0])
    same_text(hip.render_frame_sixel(there, w, h, b, spp), want, "trt_render_frame_sixel", X.search(rgb))
    same_text(hip.render_frame_sixel(there, w, h, b, spp), want, "trt_render_frame_sixel, again")
    lib, room = hip.lib(), hip.sixel_capacity(w, h)
    text, n, scene_struct = np.full(64, 0xA5, dtype=np.uint8), C.c_size_t(12345), there.as_scene()
    call = lambda sc=C.byref(scene_struct), width=w, height=h, out=text.ctypes.data, cap=room, count=C.byref(n): lib.trt_render_frame_sixel(sc, width, height, b, spp, out, cap, count)
    assert call(sc=None) == ARGUMENT and call(out=None) == ARGUMENT and call(count=None) == ARGUMENT
    assert call(width=100000, height=1, cap=1 << 40) == ARGUMENT and call(width=0) == ARGUMENT and call(height=-1) == ARGUMENT
    assert call(cap=room - 1) == CAPACITY
    assert (text == 0xA5).all() and n.value == 12345
    hip._check(hip.lib().trt_shutdown())


# ---- 3. errors, before anything is enqueued ----

def test_refusals_enqueue_nothing_and_leave_the_context_rendering(ctx):
    lib = hip.lib()
    w, h, b, spp = 41, 25, 2, 3
    rows, bad_rows = hip.RowSet.whole(w, h), hip.RowSet(0, h, h, 0, 1)
    wide, tall = hip.RowSet.whole(100000, 1), hip.RowSet.whole(1, 100000)
    cam = hip.camera_struct(anim_cameras([INDEX], w, h)[0])
    room = hip.sixel_capacity(w, h)
    mem = DeviceText(room)
    text, count = np.full(room, 0xA5, dtype=np.uint8), C.c_size_t(12345)
    p, hp, r = C.c_void_p(mem.ptr), C.c_void_p(text.ctypes.data), C.byref(rows)
    device = lambda c, camera=C.byref(cam), rs=r, bl=b, out=p, cap=room, n=C.c_void_p(mem.bytes_ptr): lib.trt_render_device_sixel(c, camera, rs, bl, spp, out, cap, n)
    hosted = lambda c, camera=C.byref(cam), rs=r, bl=b, out=hp, cap=room, n=C.byref(count): lib.trt_render_host_sixel(c, camera, rs, bl, spp, out, cap, n)
    with hip.Context(0) as empty:
        assert device(empty._h) == NO_SCENE and hosted(empty._h) == NO_SCENE
    ctx.set_scene(scene())
    h_ = ctx._h
    for entry in (device, hosted):
        for kw in (dict(c=None), dict(c=h_, out=None), dict(c=h_, n=None), dict(c=h_, camera=None), dict(c=h_, rs=None), dict(c=h_, rs=C.byref(bad_rows)),
                   dict(c=h_, bl=0), dict(c=h_, rs=C.byref(wide), cap=1 << 40), dict(c=h_, rs=C.byref(tall), cap=1 << 40)):
            assert entry(**kw) == ARGUMENT, sorted(kw)
        assert entry(h_, cap=room - 1) == CAPACITY and entry(h_, cap=0) == CAPACITY
    assert mem.untouched(ctx), "a refused device entry wrote to the caller's buffer, its guards or its length"
    assert (text == 0xA5).all() and count.value == 12345, "a refused host entry wrote to the caller's buffer or its length"
    rgb, want = oracle(w, h, INDEX, b, spp)
    assert device(h_) == 0  # the capacity to the byte
    same_text(mem.read(ctx, "the good call"), want, "the good call after the refusals", X.search(rgb))
    assert hosted(h_) == 0 and count.value == want.size
    same_text(text[:count.value], want, "the good host call after the refusals")
    assert (text[count.value:] == 0xA5).all(), "the host entry wrote behind the length it reports"


# ---- 4. the delta entries are undisturbed ----

def test_an_image_leaves_the_delta_entries_shown_frame_alone():
    w, h, b, spp = 41, 25, 2, 3
    rows = hip.RowSet.whole(w, h)
    cams = anim_cameras([7, 33], w, h)
    with hip.Context(0) as c:
        c.set_scene(scene())
        assert c.render_host_ansi_delta(cams[0], rows, b, spp).size == hip.ansi_bytes(w, h)  # a keyframe
        same_text(c.render_host_sixel(cams[1], rows, b, spp), oracle(w, h, 33, b, spp)[1], "the image of another camera")
        same_text(device_sixel(c, cams[1], w, h, b, spp, offset=1), oracle(w, h, 33, b, spp)[1], "the device entry")
        assert c.render_host_ansi_delta(cams[0], rows, b, spp).size == 0, "the shown frame changed under an image"
        moved = c.render_host_ansi_delta(cams[1], rows, b, spp).size
        assert 0 < moved < hip.ansi_bytes(w, h), "a delta, not a keyframe, behind an image"
        same_text(c.render_host_sixel(cams[0], rows, b, spp), oracle(w, h, 7, b, spp)[1], "an image behind a delta")
        assert c.render_host_ansi_delta(cams[1], rows, b, spp).size == 0


# ---- 5. the demo ----

def test_demo_program_writes_one_image_per_frame(tmp_path):
    """examples/trt_demo --sixel: trt_render_frame_sixel into a buffer of trt_sixel_capacity, one fwrite of the reported length per frame and
    nothing else on stdout -- three texts, each of which the structural reader takes for a 160 x 48 picture, the first the palette indices of
    the frame --rgb8 wrote"""
    exe = os.path.join(T.ROOT, "examples", "trt_demo")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", T.ROOT, "demo"])
    sky = tmp_path / "colors"
    sky.mkdir()
    for f in T.FACES:
        (sky / (f + ".ppm")).write_bytes(T.golden_ppm_raw("colors", f))
    run = subprocess.run([exe, str(sky), "3", "160", "48", "--sixel", "--step=0.04"], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr[-500:]
    assert b"3 frames 160x48" in run.stderr and b"as a sixel image" in run.stderr
    texts = [X.HOME + t for t in run.stdout.split(X.HOME)[1:]]
    assert len(texts) == 3 and sum(len(t) for t in texts) == len(run.stdout)
    frames = [X.read(t) for t in texts]
    assert all(f.shape == (48, 160) for f in frames) and len(np.unique(frames[0])) > 6, "a frame of one colour"
    quiet = subprocess.run([exe, str(sky), "3", "160", "48", "--sixel", "--no-draw"], capture_output=True, timeout=120)
    assert quiet.returncode == 0 and quiet.stdout == b"" and b"as a sixel image" in quiet.stderr, quiet.stderr[-500:]
    rgb8 = subprocess.run([exe, str(sky), "1", "160", "48", "--rgb8", "--step=0.04"], capture_output=True, timeout=120)
    assert rgb8.returncode == 0, rgb8.stderr[-500:]
    a = np.frombuffer(rgb8.stdout[:hip.ansi_bytes(160, 48)], dtype=np.uint8)[6:6 + (25 * 160 + 1) * 48].reshape(48, 25 * 160 + 1)[:, :25 * 160].reshape(48, 160, 25).astype(np.int32) - ord("0")
    first = np.stack([100 * a[..., at] + 10 * a[..., at + 1] + a[..., at + 2] for at in (7, 11, 15)], axis=-1).astype(np.uint8)
    assert np.array_equal(frames[0], X.search(first))
