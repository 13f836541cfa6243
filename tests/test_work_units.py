"""Work units: which sample a lane of the production kernel gets, and whether every one of them arrives.

Nothing clears the sample scratch or the framebuffer between launches, so a render that drops a unit finds the sample an earlier render
of the same frame left there.  The context of this module has trt_set_scratch_fill on: every launch first fills exactly its own samples
and exactly its own pixels with NaNs, and every frame is compared bit for bit with an oracle frame that is asserted finite first.  Each
case renders its frame twice in a row and once straight after another kernel rendered the same frame, and asserts which kernel ran.

 (a) every shipping instantiation, single frames and batches;
 (b) the queue's edges: the shapes of the unit count at which a wave's own chunk, a refill, a word per XCD or the CU cap come into play;
 (c) the split of a unit into frame, pixel, sample, row and column by multiply-high, at shapes a model of the division picks;
 (d) the RGB8 quantisation against an exact model of x86-64's cvttsd2si."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

gpu = pytest.mark.gpu
ARGUMENT = -2


# ---- the constants the cases are derived from, read from the source ----

def _source(*path):
    return open(os.path.join(T.ROOT, *path)).read()


def _number(text, pattern):
    return int(re.search(pattern, text).group(1))


_COMMON, _ROUNDS = _source("terminalraytracer_amd", "csrc", "trt_common.hpp"), _source("terminalraytracer_amd", "csrc", "trt_rounds.hpp")
assert re.search(r"kQueueChunkSamples = TRT_QUEUE_CHUNK;", _COMMON) and re.search(r"kQueueChunkSmall = TRT_QUEUE_CHUNK / TRT_QUEUE_SMALL_DIV;", _COMMON)
assert re.search(r"kPersistentBlock = TRT_BLOCK;", _COMMON) and re.search(r"kCompactBlock = TRT_COMPACT_BLOCK;", _ROUNDS)
CHUNK = _number(_COMMON, r"#define\s+TRT_QUEUE_CHUNK\s+(\d+)")                    # kQueueChunkSamples
CHUNK_SMALL = CHUNK // _number(_COMMON, r"#define\s+TRT_QUEUE_SMALL_DIV\s+(\d+)")  # kQueueChunkSmall
XCD_SHIFT = _number(_COMMON, r"kQueueXcdShift = (\d+)")
BLOCK = _number(_COMMON, r"#define\s+TRT_BLOCK\s+(\d+)")
COMPACT_BLOCK = _number(_ROUNDS, r"#define\s+TRT_COMPACT_BLOCK\s+(\d+)")
BIG_BLOCK = _number(_ROUNDS, r"kBigBlock = (\d+)")
BATCH_MAX = _number(_source("include", "trt_hip.h"), r"#define\s+TRT_BATCH_MAX\s+(\d+)")


# ---- (c) first: a model of division_magic (trt_render.hip) and of the kernels' estimate with its correction (trt_rounds.hpp) ----

def division_magic(d):
    return min((2 ** 32 + d - 1) // d, 2 ** 32 - 1)


def estimate(n, d):
    """__umulhi(n, magic(d)) for an array of n < 2^31: the raw quotient, off by at most one either way"""
    return (np.asarray(n, dtype=np.int64) * np.int64(division_magic(d))) >> np.int64(32)


def corrected(n, d):
    """(quotient, remainder) as the kernel forms them: the remainder in 32-bit arithmetic, then two selects"""
    n = np.asarray(n, dtype=np.int64)
    q = estimate(n, d)
    r = (n - q * d) & 0xFFFFFFFF
    r = (r ^ 0x80000000) - 0x80000000  # (int)(unsigned difference)
    under, over = (r < 0).astype(np.int64), (r >= d).astype(np.int64)
    return q + over - under, r + (under - over) * d


def too_small(n, d):
    n = np.asarray(n, dtype=np.int64)
    return estimate(n, d) < n // d


def too_large(n, d):
    n = np.asarray(n, dtype=np.int64)
    return estimate(n, d) > n // d


def test_the_division_model_is_divmod():
    """every d <= 4096 and seeded large ones; n at multiples of d and one either side of them, among them the largest below 2^31, and at
    the top of the range itself"""
    rng = np.random.default_rng(31)
    top = 2 ** 31 - 1
    large = np.unique(np.concatenate([rng.integers(4097, 2 ** 31 - 1, 3000), 2 ** rng.integers(12, 31, 200) + rng.integers(-2, 3, 200),
                                      [65536, 65537, 92681, 92682, 10 ** 5, 10 ** 6, top - 1, top]]))
    small_estimates = large_estimates = 0
    for d in list(range(1, 4097)) + [int(x) for x in large]:
        kmax = top // d
        ks = np.unique(np.concatenate([np.arange(0, min(kmax, 4) + 1), rng.integers(0, kmax + 1, 48), [kmax, max(kmax - 1, 0), kmax // 2]]))
        n = (ks[:, None] * d + np.array([-1, 0, 1])[None, :]).ravel()
        n = np.unique(np.concatenate([n[(n >= 0) & (n <= top)], [top, top - 1, top - d if top >= d else 0]]))
        q, r = corrected(n, d)
        assert np.array_equal(q, n // d) and np.array_equal(r, n % d), d
        small_estimates += int(too_small(n, d).sum())
        large_estimates += int(too_large(n, d).sum())
    assert too_small(np.arange(1, 100), 1).all() and not too_small([0], 1).any()  # the clipped magic of d = 1: n - 1 for every n >= 1
    assert small_estimates and large_estimates  # both corrections are exercised by the model's own check


def first_too_large(d, limit=2 ** 31 - 1, step=1 << 22):
    """the smallest n < limit whose raw estimate of n / d is one too large, or None"""
    for lo in range(0, limit, step):
        n = np.arange(lo, min(lo + step, limit), dtype=np.int64)
        hit = np.nonzero(too_large(n, d))[0]
        if hit.size:
            return int(n[hit[0]])
    return None


# ---- scenes, cameras, oracle frames (computed once, shared, never written to) ----

CAM_W, CAM_H = 96, 54


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@functools.lru_cache(maxsize=None)
def camera(index=None):
    """the stored bench camera, or camera `index` of the reference's orbit: all of one screen (a batch needs that)"""
    if index is None:
        return T.bench_camera(CAM_W, CAM_H)
    cam = np.load(os.path.join(T.GOLDEN, "cameras_anim.npz"))["camera"][index].copy()
    cam[13] = 5 * float(CAM_W) / float(CAM_H)
    return cam


@functools.lru_cache(maxsize=None)
def scene(key):
    """SYNTH-v0 spheres under the demo's two lights (one directional, one point): "s64", "s300", or "split<n>" for the split batch"""
    if key.startswith("split"):
        return S.synth_scene(int(key[5:]), T.sky("synth"), camera(), seed=17)
    return S.synth_scene({"s64": 64, "s300": 300}[key], T.sky("synth"), camera(), seed={"s64": 1234, "s300": 77}[key])


@functools.lru_cache(maxsize=None)
def oracle(key, w, h, b, spp, cam=None, band=None):
    """(frame or band of rows, (path rays, shadow rays)); the frame is asserted finite: a NaN in the expectation would hide a NaN left
    by the fill"""
    want, st = T.oracle_render(scene(key).with_camera(camera(cam)), w, h, b, spp, rows=band)
    assert np.isfinite(want).all(), (key, w, h, b, spp, cam, band)
    want.setflags(write=False)
    return want, (st.path_rays, st.shadow_rays)


def frame_rows(rows):
    lib = hip.lib()
    return [lib.trt_rowset_frame_row(C.byref(rows), i) for i in range(lib.trt_rowset_rows(C.byref(rows)))]


# ---- the kernels a case may ask for, and what the context then reports ----

REFERENCE = hip.Context.REFERENCE_ORDER
# name: (kernel, compaction, patches m, scene image, refraction with no refractor, counters)
SETTINGS = {
    "plain": (0, 0, 0, 0, False, False),
    "decoupled": (0, 1, 0, 0, False, False),
    "patches": (0, 0, 2, 0, False, False),        # 256-thread workgroups while the image fits a CU's LDS four times (s64)
    "patches_big": (0, 0, -1, 0, False, False),   # the library's own m for 128 spheres and more, 1024-thread workgroups (s300)
    "plain_image": (0, 0, 0, 1, False, False),
    "patches_image": (0, 0, 2, 1, False, False),
    "refract": (0, 0, 0, 0, True, False),
    "refract_patches": (0, 0, 2, 0, True, False),
    "reference": (REFERENCE, 0, 0, 0, False, False),
    "plain_count": (0, 0, 0, 0, False, True),
    "decoupled_count": (0, 1, 0, 0, False, True),
    "patches_count": (0, 0, 2, 0, False, True),
    "plain_image_count": (0, 0, 0, 1, False, True),
    "patches_image_count": (0, 0, 2, 1, False, True),
}


def other(variant, key="s64"):
    """the kernel that renders the same frame in between: plain -- and for plain itself the decoupled one, or where the rings do not fit beside
    the image (s300) the device-image form"""
    return "plain" if not variant.startswith("plain") or variant == "plain_image" else "decoupled" if key == "s64" else "plain_image"


def block_of(variant):
    return COMPACT_BLOCK if variant.startswith("decoupled") else BIG_BLOCK if variant == "patches_big" else BLOCK


def expected(variant):
    """(decoupled, threads per workgroup, image in device memory, m) as render_variant, render_image and path_patches report them"""
    kernel, compaction, m, image, _, _ = SETTINGS[variant]
    return (compaction == 1 and kernel == 0, block_of(variant), image == 1, 2 if m < 0 else m)


def ran(ctx):
    v = ctx.render_variant()
    return (v["decoupled"], v["workgroup_threads"], ctx.render_image()["in_device_memory"], ctx.path_patches()[0])


def configure(ctx, key, variant):
    kernel, compaction, m, image, refract, count = SETTINGS[variant]
    ctx.set_kernel(kernel)
    ctx.set_compaction(compaction)
    ctx.set_scene_image(image)
    ctx.enable_counters(count)
    if ctx.state.get("patches") != m:  # the tables are rebuilt: only when something changes
        ctx.set_path_patches(m)
        ctx.state["patches"] = m
    if ctx.state.get("scene") != key:
        ctx.set_scene(scene(key))
        ctx.state["scene"] = key
    ctx.set_refraction(np.zeros(scene(key).num_spheres) if refract else None)


def reset(ctx):
    ctx.enable_counters(False)
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_refraction(None)
    ctx.set_compaction(-1)
    ctx.set_scene_image(-1)
    if ctx.state.get("patches") != -1:  # the only table setting this module changes
        ctx.set_path_patches(-1)
    ctx.state = {"patches": -1, "scene": ctx.state.get("scene")}


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.state = {}
    try:
        c.set_scratch_fill(True)
        yield c
    finally:
        reset(c)
        c.set_scratch_fill(False)
        c.close()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(bits(got), bits(want)):
        wrong = (bits(got) != bits(want)).reshape(-1, 3).any(axis=1)
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.size} pixels differ from the oracle ({int(np.isnan(got).reshape(-1, 3).any(axis=1).sum())} of them "
                             f"left as the fill's NaN), the first at pixel {int(np.argmax(wrong))}")


def render_once(ctx, key, variant, w, h, b, spp, rows=None, cam=None):
    """one frame of `variant`: the kernel asked for ran, the frame is the oracle's, a counting form's counts are the oracle's"""
    configure(ctx, key, variant)
    rows = rows or hip.RowSet.whole(w, h)
    got = ctx.render_host(camera(cam), rows, b, spp)
    assert ran(ctx) == expected(variant), (variant, ran(ctx))
    want, counts = oracle(key, w, h, b, spp, cam)
    same(got, want[frame_rows(rows)], f"{variant} {w}x{h} spp {spp}")
    if SETTINGS[variant][5]:
        whole = rows.tile_first == 0 and rows.tile_step == 1 and rows.tile_rows >= h
        assert not whole or ctx.read_counters() == counts, (variant, ctx.read_counters(), counts)
    return got


def render_case(ctx, key, variant, w, h, b, spp, rows=None):
    """twice in a row, then once straight after another kernel rendered the same frame into the same scratch"""
    render_once(ctx, key, variant, w, h, b, spp, rows)
    render_once(ctx, key, variant, w, h, b, spp, rows)
    render_once(ctx, key, other(variant, key), w, h, b, spp, rows)
    render_once(ctx, key, variant, w, h, b, spp, rows)


# ---- (a) every shipping instantiation with the fill on ----

ON_S64 = [v for v in SETTINGS if v != "patches_big"]
ON_S300 = ["plain", "patches_big", "plain_image", "patches_image", "refract", "reference", "plain_count"]


@gpu
@pytest.mark.parametrize("key,variant", [("s64", v) for v in ON_S64] + [("s300", v) for v in ON_S300])
def test_every_instantiation_writes_every_sample_and_pixel(ctx, key, variant):
    """96x54 at three rays per pixel and an odd 67x13 at ten, whole and as a shard: the kernel named ran and wrote all of its launch"""
    try:
        render_case(ctx, key, variant, 96, 54, 4, 3)
        render_case(ctx, key, variant, 67, 13, 4, 10)
        render_case(ctx, key, variant, 67, 13, 4, 10, rows=hip.RowSet.shard(67, 13, 1, 3, 4))
    finally:
        reset(ctx)


BATCH_CAMERAS = {2: (3, 41), 3: (0, 19, 59), BATCH_MAX: tuple(range(0, 8 * BATCH_MAX, 8))[:BATCH_MAX]}


def batch_once(ctx, key, variant, w, h, b, spp, cams, launches=1):
    configure(ctx, key, variant)
    got = ctx.render_host_batch(np.array([camera(i) for i in cams]), hip.RowSet.whole(w, h), b, spp)
    assert ctx.batch_info() == (len(cams), launches), (variant, ctx.batch_info())
    assert ran(ctx) == expected(variant), (variant, ran(ctx))
    for k, i in enumerate(cams):
        same(got[k], oracle(key, w, h, b, spp, i)[0], f"{variant} batch of {len(cams)}, frame {k}, {w}x{h} spp {spp}")


def batch_case(ctx, key, variant, w, h, b, spp, cams, launches=1):
    batch_once(ctx, key, variant, w, h, b, spp, cams, launches)
    batch_once(ctx, key, variant, w, h, b, spp, cams, launches)
    batch_once(ctx, key, other(variant, key), w, h, b, spp, cams, launches)
    batch_once(ctx, key, variant, w, h, b, spp, cams, launches)


@gpu
@pytest.mark.parametrize("variant", ["plain", "patches", "decoupled"])
@pytest.mark.parametrize("n", sorted(BATCH_CAMERAS))
def test_every_batch_form_writes_every_frame(ctx, variant, n):
    """the BATCH forms, ONE launch for 2, 3 and TRT_BATCH_MAX cameras: frames 1.. of the scratch have no single-frame render to inherit from,
    frame 0 has -- all of them are filled first"""
    try:
        batch_case(ctx, "s64", variant, 67, 13, 4, 3, BATCH_CAMERAS[n])
    finally:
        reset(ctx)


SPLIT_RANGE = range(276, 300, 2)  # sphere counts near which the image of eight frames costs a workgroup that the image of one does not


@gpu
def test_a_split_batch_writes_every_frame_of_every_launch(ctx):
    """a batch of TRT_BATCH_MAX cameras that fit_batch cuts into several launches (the first sphere count in SPLIT_RANGE at which it does):
    each launch fills its own frames' samples and pixels only, and the whole batch is the oracle's, twice"""
    w, h, b, spp, cams = 32, 18, 4, 2, BATCH_CAMERAS[BATCH_MAX]
    try:
        configure(ctx, "s64", "plain")
        for spheres in SPLIT_RANGE:
            key = f"split{spheres}"
            configure(ctx, key, "plain")
            ctx.render_host_batch(np.array([camera(i) for i in cams]), hip.RowSet.whole(w, h), b, spp)
            launches = ctx.batch_info()[1]
            if launches > 1:
                break
        print(f"{spheres} spheres: a batch of {len(cams)} in {launches} launches")
        assert launches > 1, (spheres, launches)
        batch_once(ctx, key, "plain", w, h, b, spp, cams, launches)
        batch_once(ctx, key, "plain", w, h, b, spp, cams, launches)
    finally:
        reset(ctx)


# ---- (b) queue edges: one row, one ray per pixel, so that the width IS the number of work units ----

def plan(ctx, units, variant):
    """plan_render's grid and queue shape (trt_render.hip), recomputed from the occupancy trt_kernel_info reports for the kernel that just ran"""
    info = ctx.kernel_info()
    block = block_of(variant)
    cap = info["compute_units"] * max(info["max_blocks_per_cu"], 1)
    want = (units + block - 1) // block
    grid = max(1, min(want, cap))
    per_xcd = not variant.startswith("patches") and grid >= (1 << XCD_SHIFT)
    return {"grid": grid, "want": want, "cap": cap, "block": block, "words": 1 << XCD_SHIFT if per_xcd else 1, "chunk": CHUNK_SMALL if per_xcd else CHUNK}


QUEUE_VARIANTS = ["plain", "decoupled", "patches", "plain_image"]


def queue_case(ctx, variant, units):
    """... and once through the variant's counting form: a unit that two lanes trace leaves the frame right and the ray counts wrong"""
    render_once(ctx, "s64", variant + "_count", units, 1, 3, 1)
    render_case(ctx, "s64", variant, units, 1, 3, 1)
    return plan(ctx, units, variant)


@gpu
@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_fewer_units_than_a_chunk_and_a_chunk_exactly(ctx, variant):
    """1, 63, 64, 65 units (a lane, a wave short of one, a wave, a wave and a lane) and each chunk size less one, exactly, and one more:
    what is left of a wave's own chunk is served first, and the chunks behind the end of the launch hold nothing"""
    try:
        for units in (1, 63, 64, 65, CHUNK_SMALL - 1, CHUNK_SMALL, CHUNK_SMALL + 1, CHUNK - 1, CHUNK, CHUNK + 1):
            p = queue_case(ctx, variant, units)
            assert p["grid"] == (units + p["block"] - 1) // p["block"] and p["words"] == 1, (units, p)
    finally:
        reset(ctx)


@gpu
@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_one_queue_word_then_a_word_per_xcd(ctx, variant):
    """7, 8 and 9 workgroups, the last one with a single unit: one word; the first launch with a word per XCD (never with patches); words that
    serve unequal numbers of workgroups"""
    try:
        for groups in ((1 << XCD_SHIFT) - 1, 1 << XCD_SHIFT, (1 << XCD_SHIFT) + 1):
            p = queue_case(ctx, variant, (groups - 1) * block_of(variant) + 1)
            words = 1 if variant == "patches" or groups < (1 << XCD_SHIFT) else 1 << XCD_SHIFT
            assert p["grid"] == groups < p["cap"] and p["words"] == words and p["chunk"] == (CHUNK if words == 1 else CHUNK_SMALL), (groups, p)
    finally:
        reset(ctx)


@gpu
@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_as_many_units_as_the_grid_has_threads(ctx, variant):
    """grid * block units exactly, one fewer (the last lane idle from the start) and one more (another workgroup for one unit)"""
    try:
        groups, block = 12, block_of(variant)
        for units in (groups * block - 1, groups * block, groups * block + 1):
            p = queue_case(ctx, variant, units)
            assert p["grid"] == groups + (units > groups * block) < p["cap"], (units, p)
            assert (p["grid"] * p["block"] == units) == (units == groups * block)
    finally:
        reset(ctx)


@gpu
@pytest.mark.parametrize("variant", QUEUE_VARIANTS)
def test_a_capped_grid_lives_on_the_queue(ctx, variant):
    """More units than compute_units * blocks_per_cu * block: the grid is capped -- and more than its waves' OWN chunks hold, so that
    chunks that the queue hands out are inside the launch (below that, every refill lies behind the end of the launch and a wrong refill
    costs nothing): every wave refills several times, and the last chunks are partly or wholly behind the end."""
    try:
        render_once(ctx, "s64", variant, 8, 4, 3, 1)  # kernel_info describes the kernel that ran last
        p = plan(ctx, 1, variant)
        waves = p["cap"] * p["block"] // 64
        chunk = CHUNK if variant == "patches" else CHUNK_SMALL
        w, spp = 67, 13
        h = (waves * chunk * 33 // 32 + w * spp - 1) // (w * spp)  # 3 % of the units come from the queue
        h += (w * h * spp) % CHUNK == 0  # ... and the last chunk is cut by the end of the launch
        units = w * h * spp
        render_once(ctx, "s64", variant + "_count", w, h, 2, spp)  # no unit traced twice either
        render_case(ctx, "s64", variant, w, h, 2, spp)
        p = plan(ctx, units, variant)
        print(f"{variant}: {units} units, {p}")
        assert p["grid"] == p["cap"] < p["want"] and p["chunk"] == chunk, p
        assert units > p["grid"] * (p["block"] // 64) * p["chunk"] and units % p["chunk"], (units, p)
    finally:
        reset(ctx)


@gpu
@pytest.mark.parametrize("variant", ["plain", "patches", "decoupled"])
def test_chunks_that_straddle_the_frames_of_a_batch(ctx, variant):
    """67 x 13 x 3 = 2613 units a frame, a multiple of neither chunk size: chunks begin in one frame and end in the next; and 15 units a
    frame in TRT_BATCH_MAX frames: the lanes of one wave belong to more than four frames"""
    try:
        assert (67 * 13 * 3) % CHUNK and (67 * 13 * 3) % CHUNK_SMALL and 64 // 15 >= 4 and 15 * BATCH_MAX > 64
        batch_case(ctx, "s64", variant, 67, 13, 4, 3, BATCH_CAMERAS[3])
        batch_case(ctx, "s64", variant, 5, 3, 4, 1, BATCH_CAMERAS[BATCH_MAX])
    finally:
        reset(ctx)


# The ordered mean of every output kind -- doubles, the emitter's bytes, the terminal's text -- is the last kernel of its launch and
# leaves the queue armed for a launch of the same shape, which then runs no start_queue_kernel (trt_common.hpp: arm_queue).  The walk's
# queue shapes, at one ray per pixel: "wide" 64x36 = 2304 units, nine 256-thread workgroups and a word per XCD (shift 3) -- eighteen
# and twenty-seven workgroups for two and three cameras; "small" 8x4 = 32 units, ONE workgroup and one word (shift 0), for one, two or
# three cameras alike; "big" 64x36 decoupled, 1024-thread workgroups of sixteen waves, one word; the reference-order kernel, which
# neither uses nor arms the queue, in between.  (shape, cameras) in turn; the kind rotates with every launch, so a launch that finds
# the queue armed finds it armed by another kind's kernel.
ARMING_SHAPES = {"wide": ("plain", 64, 36), "small": ("plain", 8, 4), "big": ("decoupled", 64, 36), "reference": ("reference", 8, 4)}
ARMING_WALK = [("wide", 1), ("wide", 1), ("wide", 1), ("wide", 2), ("wide", 2), ("wide", 1), ("small", 1), ("small", 1), ("small", 3), ("small", 2),
               ("wide", 1), ("reference", 1), ("wide", 1), ("big", 1), ("big", 1), ("big", 2), ("big", 2), ("big", 3), ("reference", 2), ("big", 3),
               ("wide", 3), ("wide", 3), ("small", 1), ("big", 1), ("wide", 1)]


@functools.lru_cache(maxsize=None)
def arming_oracle(w, h, cam):
    """(doubles, bytes, text) of camera `cam` at 3 bounces and one ray per pixel: the oracle's frame, the checker's (int)(c*255) of it,
    the emitter's text of those bytes"""
    from test_ansi_text import emitter_text
    px = oracle("s64", w, h, 3, 1, cam)[0]
    rgb = T.oracle_rgb8(px).reshape(h, w, 3)
    text = emitter_text(rgb)
    rgb.setflags(write=False), text.setflags(write=False)
    return px, rgb, text


@gpu
def test_every_kind_arms_the_queue_once_per_launch_for_single_frames_and_batches(ctx):
    """the walk above, three times over (its length is a multiple of neither three nor two: every step meets every kind, a single camera both entries): every frame of every launch is
    bit for bit the oracle's doubles, the oracle's bytes or the emitter's text of them -- a queue left unarmed, armed for another shape or
    armed once per frame of a batch hands units out twice or not at all, which the fill's NaNs and the oracle show"""
    assert len(ARMING_WALK) % 3 and len(ARMING_WALK) % 2 and 64 * 36 >= BLOCK << XCD_SHIFT and 3 * 8 * 4 <= BLOCK and 64 * 36 < COMPACT_BLOCK << XCD_SHIFT
    cams = BATCH_CAMERAS[3]
    single = [lambda c, r: ctx.render_host(c, r, 3, 1), lambda c, r: ctx.render_host_rgb8(c, r, 3, 1), lambda c, r: ctx.render_host_ansi(c, r, 3, 1)]
    batch = [lambda c, r: ctx.render_host_batch(c, r, 3, 1), lambda c, r: ctx.render_host_batch_rgb8(c, r, 3, 1), lambda c, r: ctx.render_host_batch_ansi(c, r, 3, 1)]
    seen = set()
    try:
        for step in range(3 * len(ARMING_WALK)):
            shape, n = ARMING_WALK[step % len(ARMING_WALK)]
            variant, w, h = ARMING_SHAPES[shape]
            kind = step % 3
            what = f"step {step}: {shape} x {n} as {('doubles', 'bytes', 'text')[kind]}"
            configure(ctx, "s64", variant)
            rows = hip.RowSet.whole(w, h)
            before = ctx.launch_count()
            if n == 1 and step % 2 == 0:  # a single camera through the single-frame entry and through the batch entry in turn
                got = [single[kind](camera(cams[0]), rows)]
            else:
                got = batch[kind](np.array([camera(i) for i in cams[:n]]), rows)
                assert ctx.batch_info() == (n, n if variant == "reference" else 1), (what, ctx.batch_info())
            assert ran(ctx) == expected(variant) and ctx.launch_count() == before + 1, (what, ran(ctx))
            for k in range(n):
                want = arming_oracle(w, h, cams[k])[kind]
                if kind == 0:
                    same(got[k], want, f"{what}, frame {k}")
                else:
                    assert np.asarray(got[k]).dtype == np.uint8 and np.array_equal(np.asarray(got[k]).reshape(want.shape), want), f"{what}, frame {k}"
            seen.add((shape, n, kind))
        assert len(seen) == 3 * len(set(ARMING_WALK))
    finally:
        reset(ctx)


# ---- (c) division by multiply-high on the device, at shapes the model picks ----

def device_frame(ctx, key, variant, rows, b, spp, cam=None):
    """through trt_render_device: ONE launch whatever the frame's size (trt_render_host renders a large frame in bands, whose pixel indices start over)"""
    import torch
    configure(ctx, key, variant)
    n = len(frame_rows(rows)) * rows.width * 3
    fb = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.render_device(camera(cam), rows, b, spp, fb.data_ptr(), n * 8)
    ctx.synchronize()
    assert ran(ctx) == expected(variant), (variant, ran(ctx))
    return fb.cpu().numpy().reshape(-1, rows.width, 3)


def banded_case(ctx, key, rows, b, spp, local_band):
    """a frame too large for the oracle: the oracle renders the local rows [local_band) that the model names, the reference-order kernel the
    whole frame; the production kernel (plain, twice, then after its device-image form, which fits whatever the rays per pixel) must equal both"""
    owned = frame_rows(rows)
    r0, r1 = owned[local_band[0]], owned[local_band[1] - 1] + 1
    assert r1 - r0 == local_band[1] - local_band[0]  # the band is contiguous in the frame
    want = oracle(key, rows.width, rows.height, b, spp, None, (r0, r1))[0]
    whole = device_frame(ctx, key, "reference", rows, b, spp)
    same(whole[local_band[0]:local_band[1]], want, "reference-order kernel, the model's rows")
    assert np.isfinite(whole).all()
    for variant in ("plain", "plain", "plain_image", "plain"):
        got = device_frame(ctx, key, variant, rows, b, spp)
        same(got[local_band[0]:local_band[1]], want, f"{variant}, the model's rows")
        same(got, whole, f"{variant} against the reference-order kernel")


@gpu
def test_an_estimate_one_too_small_is_corrected_for_a_divisor_of_one(ctx):
    """d = 1 clips the magic to 2^32 - 1: the raw estimate is n - 1 for every n >= 1.  One ray per pixel (every case of (b) as well); a
    frame one pixel wide, 300 rows; a shard of tiles one row high."""
    try:
        assert too_small(np.arange(1, 300 * 2), 1).all()
        for variant in QUEUE_VARIANTS:
            render_case(ctx, "s64", variant, 1, 300, 3, 2)                                       # width 1
            render_case(ctx, "s64", variant, 16, 9, 3, 1)                                        # spp 1
            render_case(ctx, "s64", variant, 16, 9, 3, 3, rows=hip.RowSet.shard(16, 9, 1, 4, 1))  # tile_rows 1, not dealt from tile 0 with step 1
    finally:
        reset(ctx)


@functools.lru_cache(maxsize=None)
def spp_shape():
    """1000 rays per pixel (e = 1000 * 4294968 - 2^32 = 704): the smallest frame 80 pixels wide with a unit whose estimate is too large"""
    spp, w = 1000, 80
    first = first_too_large(spp, 2 ** 26)
    h = first // spp // w + 1
    wrong = np.nonzero(too_large(np.arange(w * h * spp), spp))[0]
    rows = wrong // spp // w
    return spp, w, h, int(rows.min()), int(rows.max()) + 1, int(wrong.size)


def test_the_model_finds_the_frame_whose_rays_per_pixel_are_overestimated():
    spp, w, h, r0, r1, wrong = spp_shape()
    assert wrong >= 1 and 0 <= r0 < r1 <= h and h <= 128 and w * h * spp < 2 ** 31 - 1
    assert not too_large(np.arange(w * (h - 1) * spp), spp).any()  # the smallest such frame of that width


@gpu
def test_an_estimate_one_too_large_is_corrected_for_the_rays_per_pixel(ctx):
    """unit -> (pixel, k): with 1000 rays per pixel the estimate of the pixel is one too large from about unit 6.1 million on (n e >= 2^32
    with e = 704), for units whose k is close to 999"""
    spp, w, h, r0, r1, wrong = spp_shape()
    assert wrong >= 1
    try:
        banded_case(ctx, "s64", hip.RowSet.whole(w, h), 2, spp, (r0, r1))
    finally:
        reset(ctx)


@functools.lru_cache(maxsize=None)
def width_shape():
    """a frame 1000 pixels wide: the estimate of the row is one too large from about pixel 6.1 million on, in the last columns"""
    w = 1000
    first = first_too_large(w, 2 ** 26)
    h = first // w + 1
    wrong = np.nonzero(too_large(np.arange(w * h), w))[0]
    return w, h, int((wrong // w).min()), int((wrong // w).max()) + 1, int(wrong.size)


@gpu
def test_an_estimate_one_too_large_is_corrected_for_the_width(ctx):
    """pixel -> (row, column) at one ray per pixel, a frame of 1000 x 6100-odd pixels in ONE launch"""
    w, h, r0, r1, wrong = width_shape()
    assert wrong >= 1 and w * h < 2 ** 23
    try:
        banded_case(ctx, "s64", hip.RowSet.whole(w, h), 2, 1, (max(0, r0 - 1), r1))
    finally:
        reset(ctx)


@functools.lru_cache(maxsize=None)
def tile_shape():
    """the smallest tile height d for which local row d - 1 -- the last row of the first tile -- is overestimated: (d - 1) e >= 2^32"""
    for d in range(65537, 200000):
        if too_large([d - 1], d)[0]:
            wrong = np.nonzero(too_large(np.arange(d), d))[0]
            return d, int(wrong.min()), int(wrong.max()) + 1
    raise AssertionError("no such tile height")


@gpu
def test_an_estimate_one_too_large_is_corrected_for_the_tile_rows(ctx):
    """local row -> (tile, row of the tile), used by rowsets that are not dealt from tile 0 with step 1.  n e >= 2^32 needs n >= 2^32 / e with
    e < tile_rows, so tiles and shards of more than 65536 rows: far from any frame, but within the 2^31 pixel limit for a narrow one (the
    limit alone does not put the one-too-large branch out of reach).  Rank 1 of 2 of a frame one pixel wide and 2 d rows high, d the
    smallest tile height the model finds: its last local rows are overestimated."""
    d, n0, n1 = tile_shape()
    rows = hip.RowSet.shard(1, 2 * d, 1, 2, d)
    assert n1 == d and too_large(np.arange(n0, n1), d).all() and hip.lib().trt_rowset_rows(C.byref(rows)) == d
    try:
        banded_case(ctx, "s64", rows, 2, 1, (max(0, n0 - 2), n1))
    finally:
        reset(ctx)


@functools.lru_cache(maxsize=None)
def batch_shape():
    """units per frame d = w * h between 2 10^4 and 10^5 for which a unit of a batch of 8 is put one frame too far: (8 d - 1) e >= 2^32"""
    for d in range(20000, 100001):
        if d % 160 == 0 and too_large([BATCH_MAX * d - 1], d)[0]:
            return 160, d // 160, d
    raise AssertionError("no such frame")


def test_the_model_finds_the_batch_whose_frames_are_overestimated():
    w, h, d = batch_shape()
    e = d * division_magic(d) - 2 ** 32
    assert 20000 <= d <= 100000 and w * h == d and BATCH_MAX * d * e >= 2 ** 32
    assert too_large(np.arange(BATCH_MAX * d), d).any() and not too_small(np.arange(BATCH_MAX * d), d).any()


@gpu
@pytest.mark.parametrize("variant", ["plain", "patches", "decoupled"])
def test_an_estimate_one_too_large_is_corrected_for_the_frames_of_a_batch(ctx, variant):
    """unit -> (frame, unit of the frame): the last units of the later frames of TRT_BATCH_MAX are estimated into the frame behind theirs;
    compared with the oracle in full"""
    w, h, d = batch_shape()
    wrong = np.nonzero(too_large(np.arange(BATCH_MAX * d), d))[0]
    assert wrong.size and (wrong // d).max() == BATCH_MAX - 1
    try:
        batch_case(ctx, "s64", variant, w, h, 2, 1, BATCH_CAMERAS[BATCH_MAX])
    finally:
        reset(ctx)


@gpu
def test_a_frame_rendered_in_bands_on_two_streams_is_filled_per_band(ctx):
    """trt_render_host renders a whole frame of 32 MB or more in four bands, odd ones on a second stream with a scratch of its own: each band
    fills its own samples and its own rows of the framebuffer.  The oracle renders the rows either side of every band edge, the
    reference-order kernel (one launch through trt_render_device) the whole frame."""
    w, h, b, spp = 1400, 1000, 2, 1
    assert w * h * 24 >= 32 << 20 and h >= 256
    edges = [(0, 2), (248, 252), (498, 502), (748, 752), (h - 2, h)]
    try:
        whole = device_frame(ctx, "s64", "reference", hip.RowSet.whole(w, h), b, spp)
        for variant in ("plain", "plain", "decoupled", "plain"):
            configure(ctx, "s64", variant)
            before = ctx.launch_count()
            got = ctx.render_host(camera(), hip.RowSet.whole(w, h), b, spp)
            assert ran(ctx) == expected(variant) and ctx.launch_count() - before == 4  # a launch per band
            for r0, r1 in edges:
                same(got[r0:r1], oracle("s64", w, h, b, spp, None, (r0, r1))[0], f"{variant}, rows {r0}..{r1}")
            same(got, whole, f"{variant} against the reference-order kernel")
    finally:
        reset(ctx)


@gpu
def test_2_to_the_31_units_are_refused_and_the_context_renders_on(ctx):
    """1000 x 1000 pixels at 2148 rays per pixel are 2^31 - 1 units or more, and so are two frames at 1074: TRT_ERR_ARGUMENT, nothing launched"""
    rows = hip.RowSet.whole(1000, 1000)
    assert 1000 * 1000 * 2148 >= 2 ** 31 - 1 > 1000 * 1000 * 2147 and 2 * 1000 * 1000 * 1074 >= 2 ** 31 - 1 > 1000 * 1000 * 1074
    try:
        configure(ctx, "s64", "plain")
        with pytest.raises(hip.TrtError) as e:
            ctx.render_host(camera(), rows, 2, 2148)
        assert e.value.code == ARGUMENT and "work units" in str(e.value)
        with pytest.raises(hip.TrtError) as e:
            ctx.render_host_batch(np.array([camera(0), camera(19)]), rows, 2, 1074)
        assert e.value.code == ARGUMENT and "work units" in str(e.value)
        render_case(ctx, "s64", "plain", 67, 13, 4, 10)
        batch_once(ctx, "s64", "plain", 67, 13, 4, 3, BATCH_CAMERAS[2])
    finally:
        reset(ctx)


# ---- (d) quantisation ----

def quantize_model(c):
    """(unsigned char)d2i(c * 255): the product in double precision; truncated toward zero while its magnitude is below 2^31, otherwise
    (NaN included) x86-64's integer indefinite 0x80000000; the low byte"""
    with np.errstate(all="ignore"):
        p = np.asarray(c, dtype=np.float64) * 255.0
        ok = np.abs(p) < 2147483648.0
        t = np.where(ok, np.trunc(np.where(ok, p, 0.0)), -2147483648.0).astype(np.int64)
    return (t & 0xFF).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def quantize_inputs():
    k = np.arange(256, dtype=np.float64) / 255.0
    edge = 2147483648.0 / 255.0
    around = lambda x: [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]
    special = np.concatenate([
        np.nextafter(k, -np.inf), k, np.nextafter(k, np.inf),                      # k / 255 and its neighbours
        [0.0, -0.0, 1.0, 1.5, 2.0, 256.0 / 255.0, 257.0 / 255.0, 3.999, 1000.25, 65536.0, 1e6, 8421504.6],  # above 1: modulo 256
        -k[1:], [-0.001, -0.5, -1.0, -1.0 / 255.0, -1.004, -300.7, -1e6],              # negative
        around(edge), around(-edge), around(np.nextafter(edge, 0.0)),                 # +-2^31 / 255
        [-8421504.0 - 128.0 / 255.0, -2147483648.0 / 255.0, -8421504.6, -8421505.0, -1e10, 1e10, 1e300, -1e300],
        [np.inf, -np.inf, np.nan, -np.nan],
        [5e-324, -5e-324, 2.2250738585072014e-308, 1e-310, -1e-310, 2.2250738585072009e-308],  # denormals and the smallest normal
    ])
    rng = np.random.default_rng(255)
    n = 1 << 20
    spread = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-1074, 1024, n)) * rng.choice([-1.0, 1.0], n)
    near = rng.uniform(-2.0, 260.0, n // 4) / 255.0  # ... and a quarter as many where the bytes are
    special.setflags(write=False)
    return special, np.concatenate([spread, near])


def test_the_quantisation_model_knows_its_edges():
    special, seeded = quantize_inputs()
    assert special.size >= 257 * 3 and seeded.size >= 1 << 20
    p = special * 255.0
    with np.errstate(all="ignore"):
        assert (p == -2147483648.0).any() and (p == 2147483648.0).any() and (p < -2147483648.0).any() and np.isnan(p).any()
        assert (np.abs(seeded * 255.0) >= 2147483648.0).any() and (np.abs(seeded * 255.0) < 1.0).any()
    m = quantize_model(np.array([0.0, -0.0, 1.0, 256.0 / 255.0, -1.0 / 255.0, np.nan, np.inf, -2147483648.0 / 255.0, 2147483648.0 / 255.0, 0.5]))
    assert m.tolist() == [0, 0, 255, 0, 255, 0, 0, 0, 0, 127]
    assert np.array_equal(quantize_model(np.arange(256) / 255.0), T.oracle_rgb8(np.arange(258)[:, None].repeat(3, 1) / 255.0)[:256, 0])


@gpu
def test_quantize_device_is_cvttsd2si_on_every_kind_of_double(ctx):
    """trt_quantize_device against the model: +-0, k / 255 and its neighbours, values above 1 and below 0, +-2^31 / 255 and their neighbours, a
    product of exactly -2^31 and beyond, infinities, NaN, denormals, 2^20 seeded values over all exponents; 1, 85, 86 and 257 pixels (255,
    258 and 771 values: a workgroup less a thread, one and two threads, three and three threads) and all of them; nothing behind the end"""
    import torch
    special, seeded = quantize_inputs()
    everything = np.concatenate([special, seeded])
    for values in (special[:3], special[:85 * 3], special[:86 * 3], special[:257 * 3], special[:special.size // 3 * 3], everything[:everything.size // 3 * 3]):
        pixels = values.size // 3
        src = torch.from_numpy(values.copy()).to("cuda:0")
        dst = torch.full((values.size + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        ctx.quantize_device(src.data_ptr(), pixels, dst.data_ptr())
        ctx.synchronize()
        got = dst.cpu().numpy()
        want = quantize_model(values)
        wrong = np.nonzero(got[:values.size] != want)[0]
        assert wrong.size == 0, (pixels, wrong.size, [(float(values[i]), int(got[i]), int(want[i])) for i in wrong[:8]])
        assert (got[values.size:] == 0xA5).all(), pixels
