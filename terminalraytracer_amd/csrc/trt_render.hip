// trt_render.hip -- render dispatch: which instantiation of the production kernel (csrc/trt_rounds.hpp) a launch runs -- a single
// frame, or several cameras of one scene (a single frame is a batch of one) -- its plan and its launch, occupancy, the copy-out to
// the host, kernel times and resource usage.
// Compiled for gfx950 only, with -ffp-contract=off (see trt_device.hpp).
#define TRT_UNIT_RENDER 1 // this unit is the home of the kernels that are not templates (trt_common.hpp, trt_simple.hpp)
#include "trt_context.hpp"
#ifndef TRT_REDUCE_BLOCK
#define TRT_REDUCE_BLOCK 64 // one wave: fits beside the render kernels of the frames in flight wherever a wave retires (+0.8 % decoupled)
#endif
#include "trt_simple.hpp"
#include "trt_ansi.hpp"
#include "trt_ansi_delta.hpp"
#include "trt_ansi256.hpp"
#include "trt_ansi_half.hpp"
#include "trt_kitty.hpp"
#include "trt_sixel.hpp"

using namespace trt_impl;

namespace trt_impl
{

// ---- which kernel a frame runs ----
// The production kernel's instantiations (render_rounds_kernel<COUNT, REFRACT, COMPACT, PATCHES, BIG, DEVICE_IMAGE, BATCH, SPECULAR, SKY_FILTER>), each with its
// counting form where it has one (the rays trt_read_counters reports), and the reference-order kernel (trt_set_kernel(1)).
enum Variant : int
{
    kPlain, kPlainCount,
    kPatches, kPatchesCount,     // a family per patch of a sphere (trt_raygrid.h)
    kPatchesBig,                 // ... in 1024-thread workgroups: one LDS image for sixteen waves
    kDecoupled, kDecoupledCount, // the shading decoupled from the owning lane (COMPACT, trt_rounds.hpp): rings in LDS
    kRefract, kRefractCount, kRefractPatches, kRefractPatchesCount, // the refraction extension (parity unpinned)
    kPlainImage, kPlainImageCount, kPatchesImage, kPatchesImageCount, // the plain rounds with the scene image in device memory (DEVICE_IMAGE)
    kSpecular, kSpecularCount, kSpecularPatches, kSpecularPatchesCount, // the specular extension (parity unpinned)
    kSkyFilter, kSkyFilterCount, kSkyFilterPatches, kSkyFilterPatchesCount, // bilinear sky filtering (parity unpinned)
    kReference,                  // render_simple_kernel: one thread per pixel; not in kRounds
    kReferenceImage,             // ... reading the scene's records from device memory
};

using RoundsKernel = void (*)(trt::SceneView, trt::CullView, trt::FrameView, trt::GridView);
// The BATCH form of an instantiation (trt_rounds.hpp; several cameras of one scene per launch, trt_render_device_batch): plain,
// patches, decoupled -- the non-counting instantiations with the image in LDS.  Everything else a context may be set to render
// is served one launch per camera.
using BatchKernel = void (*)(trt::SceneView, trt::CullView, trt::FrameView, trt::GridView, trt::BatchView);
struct RoundsVariant
{
    RoundsKernel fn;
    int block;  // threads per workgroup
    bool rings; // LDS: the image, then a shading ring per wave (compact_lds_bytes); otherwise the image alone
    bool image; // the image in device memory (stage_image_kernel), no dynamic LDS
    BatchKernel batch; // null: no BATCH form
};
static const RoundsVariant kRounds[kReference] = {
    {trt::render_rounds_kernel<false>, trt::kPersistentBlock, false, false, trt::render_rounds_kernel<false, false, false, false, false, false, true, false, false, trt::BatchView>},
    {trt::render_rounds_kernel<true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, false, false, true>, trt::kPersistentBlock, false, false, trt::render_rounds_kernel<false, false, false, true, false, false, true, false, false, trt::BatchView>},
    {trt::render_rounds_kernel<true, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, false, false, true, true>, trt::kBigBlock, false},
    {trt::render_rounds_kernel<false, false, true>, trt::kCompactBlock, true, false, trt::render_rounds_kernel<false, false, true, false, false, false, true, false, false, trt::BatchView>},
    {trt::render_rounds_kernel<true, false, true>, trt::kCompactBlock, true},
    {trt::render_rounds_kernel<false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<true, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, true, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<true, true, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, false, false, false, false, true>, trt::kPersistentBlock, false, true},
    {trt::render_rounds_kernel<true, false, false, false, false, true>, trt::kPersistentBlock, false, true},
    {trt::render_rounds_kernel<false, false, false, true, false, true>, trt::kPersistentBlock, false, true},
    {trt::render_rounds_kernel<true, false, false, true, false, true>, trt::kPersistentBlock, false, true},
    {trt::render_rounds_kernel<false, false, false, false, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<true, false, false, false, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, false, false, true, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<true, false, false, true, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, false, false, false, false, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<true, false, false, false, false, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<false, false, false, true, false, false, false, false, true>, trt::kPersistentBlock, false},
    {trt::render_rounds_kernel<true, false, false, true, false, false, false, false, true>, trt::kPersistentBlock, false},
};
static_assert(TRT_BATCH_MAX == kEyeSlots && TRT_BATCH_MAX == trt::kBatchMax, "a frame of a batch has an eye slot of the scene's tables and a place in BatchView");

static BatchKernel batch_form(Variant v)
{
    return v < kReference ? kRounds[v].batch : nullptr;
}

static bool image_in_device_memory(Variant v)
{
    return v == kReferenceImage || (v < kReference && kRounds[v].image);
}

// Does a frame of `spp` rays per pixel read its scene image from device memory (trt_set_scene_image)?  Automatic: only when the
// image of the kernel it runs does not fit LDS, so that every scene that fits runs what it ran before there was a device image.
static bool wants_device_image(const trt_context *ctx, int spp)
{
    if (ctx->scene_image >= 0)
        return ctx->scene_image == 1;
    return (ctx->kernel == 1 ? scene_lds_bytes(ctx->scene) : image_lds_bytes(ctx, spp)) > (size_t)ctx->lds_limit;
}

constexpr int kCompactionMinLights = 2; // trt_set_compaction(-1): decouple the shading from two lights up (with one it is a wash)

// Is a frame of `units` samples on this context decoupled?  Measured (profiles/r02/n_compaction.md): 6 % faster with the two lights
// of the BASELINE scenes, 10 / 12 / 15 / 17 % with 3 / 4 / 6 / 8; the ring costs about what one light's idle lanes cost.  Its
// 1024-thread workgroups hold a whole CU until their last wave retires, which pipelined frames feel on SMALL launches
// (profiles/r02/t_shards.txt: a 1/8 shard of the 1080p frame, three in flight, 0.249 ms decoupled against 0.218 plain; half a
// frame 0.884 against 0.871; the whole frame 1.630 against 1.685): by default only launches of 16 M samples or more are decoupled.
constexpr long kCompactionMinUnits = 16L << 20;

static bool renders_decoupled(const trt_context *ctx, long units)
{
    if (!ctx->have_scene || ctx->compact_blocks_per_cu <= 0 || ctx->compaction == 0)
        return false;
    // ... and only scenes whose path rays are served by tables: with the few spheres of a scene that sweeps (BASELINE configs[1]:
    // 8 spheres, most rays end on the ground or the sky) the ring costs more than the idle lanes (round 4, final kernel,
    // profiles/r04/i_all_configs_one_gpu.md: 43.3 G path rays/s plain against 40.8 decoupled; config 3 equal, config 4 +4 % decoupled)
    const bool pays = ctx->scene.num_dir + ctx->scene.num_point >= kCompactionMinLights && units >= kCompactionMinUnits && ctx->grids.path_enabled &&
                      ctx->compact_blocks_per_cu * trt::kCompactBlock >= ctx->rounds_blocks_per_cu * trt::kPersistentBlock;
    return ctx->compaction > 0 || pays;
}

// do the scene's spheres have patches?  (larger tables: one queue word, never decoupled)
static bool has_patches(const trt_context *ctx)
{
    return ctx->grids.path_enabled && ctx->grids.patch_m > 0;
}

// Which kernel a launch of `frames` cameras and `units` samples in all runs.  A batch of 1/8 shards is a large launch: the
// decoupling threshold sees the whole launch's units, and the rings must fit beside the image of all its frames.  Whether the
// image goes to device memory is asked of ONE frame: a batch that does not fit LDS is split (fit_batch), not moved.
static Variant choose_variant(const trt_context *ctx, long units, int spp, int frames = 1)
{
    const bool device_image = wants_device_image(ctx, spp);
    if (ctx->kernel == 1)
        return device_image ? kReferenceImage : kReference;
    const bool count = ctx->counters_enabled;
    const bool patches = has_patches(ctx);
    if (ctx->ior_count) // no device-image form: a scene whose image does not fit LDS fails at render time
        return patches ? (count ? kRefractPatchesCount : kRefractPatches) : (count ? kRefractCount : kRefract);
    if (ctx->specular) // the same: the plain rounds with the image in LDS, one launch per camera, never decoupled
        return patches ? (count ? kSpecularPatchesCount : kSpecularPatches) : (count ? kSpecularCount : kSpecular);
    if (ctx->sky_filter) // the same again
        return patches ? (count ? kSkyFilterPatchesCount : kSkyFilterPatches) : (count ? kSkyFilterCount : kSkyFilter);
    if (device_image)
        return patches ? (count ? kPatchesImageCount : kPatchesImage) : (count ? kPlainImageCount : kPlainImage);
    // scenes whose spheres have patches (dense ones) run the plain rounds; the rings must fit beside the image (the occupancy
    // figures were taken for 64 rays per pixel: with more, the jitter table may push the rings out of LDS)
    if (!patches && renders_decoupled(ctx, units) && compact_lds_bytes(ctx, spp, frames) <= (size_t)ctx->lds_limit)
        return count ? kDecoupledCount : kDecoupled;
    if (!patches)
        return count ? kPlainCount : kPlain;
    // sixteen waves around ONE image when they are more than the 256-thread workgroups that fit the CU's LDS hold
    const bool big = ctx->big_blocks_per_cu * trt::kBigBlock > ctx->rounds_blocks_per_cu * trt::kPersistentBlock;
    return count ? kPatchesCount : big ? kPatchesBig : kPatches;
}

// the variant trt_render_variant / trt_kernel_info describe: the most recent launch's; before the first, a whole large frame's
static Variant described_variant(const trt_context *ctx)
{
    return ctx->last_variant >= 0 ? (Variant)ctx->last_variant : choose_variant(ctx, kCompactionMinUnits, 64);
}

static int described_spp(const trt_context *ctx)
{
    return ctx->last_variant >= 0 ? ctx->last_spp : 64;
}

// dynamic LDS of a launch of `frames` frames of variant v
static size_t launch_lds_bytes(const trt_context *ctx, Variant v, int spp, int frames = 1)
{
    const RoundsVariant &k = kRounds[v];
    return k.image ? 0u : k.rings ? compact_lds_bytes(ctx, spp, frames) : image_lds_bytes(ctx, spp, frames);
}

// Workgroups per CU a launch of variant v is sized by.  The single-frame instantiations: what refresh_occupancy stored for the
// scene (every 256-thread variant with the image in LDS by the plain instantiation's occupancy).  The BATCH forms, whose image grows
// with the frames of the launch: their own occupancy with `lds` bytes of dynamic LDS (0: it does not fit), asked once per size.
static int blocks_per_cu(trt_context *ctx, Variant v, bool batch, size_t lds, int *blocks)
{
    const RoundsVariant &k = kRounds[v];
    if (!batch)
    {
        *blocks = k.image ? ctx->device_blocks_per_cu : k.rings ? ctx->compact_blocks_per_cu : k.block == trt::kBigBlock ? ctx->big_blocks_per_cu : ctx->rounds_blocks_per_cu;
        return TRT_OK;
    }
    for (const trt_context::BatchOccupancy &o : ctx->batch_occupancy)
        if (o.kernel == (const void *)k.batch && o.lds == lds)
        {
            *blocks = o.blocks;
            return TRT_OK;
        }
    *blocks = 0;
    if (lds <= (size_t)ctx->lds_limit)
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k.batch, k.block, lds));
    if (ctx->batch_occupancy.size() >= 64)
        ctx->batch_occupancy.clear();
    ctx->batch_occupancy.push_back({(const void *)k.batch, lds, *blocks});
    return TRT_OK;
}

struct RenderPlan
{
    Variant variant;
    bool batch; // the variant's BATCH form
    unsigned grid, block;
    size_t lds;        // dynamic LDS bytes
    unsigned ring_at;  // kDecoupled*: FrameView::ring_at
    unsigned queue_shift, chunk; // FrameView::queue_shift, chunk
    int per_cu;        // workgroups per CU the grid was sized by, before it is made at least one (0: the launch's LDS does not fit)
};

// The launch of `frames` frames of `units` samples in all -- a single frame, or `batch`: the BATCH form of what they run: the
// production kernel's workgroups fill the context's CUs as far as the units need them.
static int plan_render(trt_context *ctx, long units, int spp, int frames, bool batch, RenderPlan *plan)
{
    const Variant v = choose_variant(ctx, units, spp, frames);
    if (v == kReference || v == kReferenceImage)
    {
        *plan = RenderPlan{v, false, (unsigned)((units / spp + 255) / 256), 256u, v == kReference ? scene_lds_bytes(ctx->scene) : 0u};
        return TRT_OK;
    }
    const RoundsVariant &k = kRounds[v];
    RenderPlan p{v, batch, 0u, (unsigned)k.block, launch_lds_bytes(ctx, v, spp, frames), k.rings ? (unsigned)compact_ring_at(ctx, spp, frames) : 0u};
    const int rc = blocks_per_cu(ctx, v, batch, p.lds, &p.per_cu);
    if (rc)
        return rc;
    const long cap = (long)(ctx->compute_units - (ctx->stream == ctx->own_stream ? ctx->reserved_cus : 0)) * std::max(p.per_cu, 1);
    const long want = (units + k.block - 1) / k.block;
    p.grid = (unsigned)std::max(1L, std::min(want, cap));
    // The queue (trt_common.hpp, kQueueStride): a word per XCD and chunks of half the size for scenes whose tables are small enough
    // that a wave may change its place in the image twice as often (no patches), when every word has workgroups; otherwise one
    // word.  Every wave owns its first chunk without asking.
    const bool per_xcd = !has_patches(ctx) && p.grid >= (1u << trt::kQueueXcdShift);
    p.queue_shift = per_xcd ? (unsigned)trt::kQueueXcdShift : 0u;
    p.chunk = per_xcd ? trt::kQueueChunkSmall : trt::kQueueChunkSamples;
    *plan = p;
    return TRT_OK;
}

// workgroups of a variant that fit one CU at the LDS of a frame of 64 rays per pixel
static hipError_t occupancy(const trt_context *ctx, Variant v, int *blocks)
{
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, kRounds[v].fn, kRounds[v].block, launch_lds_bytes(ctx, v, 64));
}

// The production kernel's occupancy depends on the scene and its tables only through the size of the LDS image: queried once
// per size, not once per frame.  The instantiations that read the image from device memory have no dynamic LDS: their occupancy,
// queried once, sizes the launches of scenes whose image does not fit (trt_set_scene_image(ctx, 0): those fail, as they did
// before there was a device image).
int refresh_occupancy(trt_context *ctx)
{
    const trt::SceneView &v = ctx->scene;
    const size_t lds_need = std::max(scene_lds_bytes(v), image_lds_bytes(ctx, 64));
    if (lds_need > (size_t)ctx->lds_limit && ctx->scene_image == 0)
        return fail(TRT_ERR_CAPACITY, "scene needs %zu B of LDS staging, device offers %d", lds_need, ctx->lds_limit);
    if (ctx->device_blocks_per_cu == 0)
    {
        int blocks = 0;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kRounds[kPlainImage].fn, kRounds[kPlainImage].block, 0));
        ctx->device_blocks_per_cu = std::max(blocks, 1);
    }
    if (ctx->occupancy_for_lds != image_lds_bytes(ctx, 64))
    {
        const bool fits = image_lds_bytes(ctx, 64) <= (size_t)ctx->lds_limit;
        int blocks = 0;
        if (fits)
            HIP_TRY(occupancy(ctx, kPlain, &blocks));
        ctx->rounds_blocks_per_cu = std::max(blocks, 1);
        ctx->occupancy_for_lds = image_lds_bytes(ctx, 64);
        ctx->compact_blocks_per_cu = 0;
        if (compact_lds_bytes(ctx, 64) <= (size_t)ctx->lds_limit)
            HIP_TRY(occupancy(ctx, kDecoupled, &ctx->compact_blocks_per_cu));
        ctx->big_blocks_per_cu = 0;
        if (fits && ctx->rounds_blocks_per_cu < 4) // the image no longer fits four times: one image for sixteen waves instead
            HIP_TRY(occupancy(ctx, kPatchesBig, &ctx->big_blocks_per_cu));
    }
    return TRT_OK;
}

int prepare_jitter(trt_context *ctx, const Camera *cam, int width, int height, int spp)
{
    // TRT.c:981-982, :992-993: triangle_wave(2*PI*k/spp)/2*pixel_width and triangle_wave(PI*k/spp)/2*pixel_height
    const double pw = cam->screen_width / width, ph = cam->screen_height / height;
    if (ctx->jit_spp == spp && ctx->jit_pw == pw && ctx->jit_ph == ph)
        return TRT_OK;
    std::vector<double> j(2 * (size_t)spp);
    for (int k = 0; k < spp; k++)
    {
        j[k] = triangle_wave(2 * kPi * k / spp) / 2 * pw;
        j[spp + k] = triangle_wave(kPi * k / spp) / 2 * ph;
    }
    HIP_TRY(ctx->d_jitter.reserve(j.size()));
    HIP_TRY(hipStreamSynchronize(ctx->stream)); // a frame in flight may still read the old table
    HIP_TRY(hipMemcpy(ctx->d_jitter.ptr, j.data(), j.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->jit_spp = spp;
    ctx->jit_pw = pw;
    ctx->jit_ph = ph;
    return TRT_OK;
}

// TRT.c:987-988 without the jitter: one value per column and one per frame row, formed on the host in the
// reference's operation order (this file is compiled with -ffp-contract=off for host and device alike)
int prepare_axes(trt_context *ctx, const Camera *cam, int width, int height)
{
    const double sw = cam->screen_width, sh = cam->screen_height;
    if (ctx->axes_w == width && ctx->axes_h == height && ctx->axes_sw == sw && ctx->axes_sh == sh)
        return TRT_OK;
    std::vector<double> t((size_t)width + height);
    for (int column = 0; column < width; column++)
        t[column] = (((double)column / (double)width) * sw - sw / 2.0);
    for (int row = 0; row < height; row++)
        t[(size_t)width + row] = -(((double)row / (double)height) * sh - sh / 2.0);
    HIP_TRY(ctx->d_axes.reserve(t.size()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(ctx->d_axes.ptr, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->axes_w = width;
    ctx->axes_h = height;
    ctx->axes_sw = sw;
    ctx->axes_sh = sh;
    return TRT_OK;
}

void allow_large_lds_render(const trt_context *ctx)
{
    (void)hipFuncSetAttribute((const void *)trt::render_simple_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::render_simple_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::render_simple_kernel<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    for (const RoundsVariant &k : kRounds)
    {
        if (!k.image)
            (void)hipFuncSetAttribute((const void *)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
        if (k.batch)
            (void)hipFuncSetAttribute((const void *)k.batch, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    }
}

// The scene image of a frame in device memory, for render_rounds_kernel<.., DEVICE_IMAGE>: one workgroup, since fill_image has
// barriers between its phases.  It holds the frame's camera, jitter and the eye's families, so it is written on the frame's
// stream in front of every launch that reads it.
constexpr int kImageBlock = 1024;
__global__ __launch_bounds__(kImageBlock) void stage_image_kernel(trt::SceneView s, trt::CullView cull, trt::FrameView f, trt::GridView grids)
{
    trt::fill_image(trt::image_layout(const_cast<double *>(f.image), s.num_spheres, s.num_dir, s.num_point, cull.padded, f.spp), s, cull, f, grids);
}

} // namespace trt_impl

extern "C" int trt_enable_counters(trt_context *ctx, int enable)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    ctx->counters_enabled = enable != 0;
    return TRT_OK;
}

extern "C" int trt_set_scratch_fill(trt_context *ctx, int on)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    ctx->scratch_fill = on != 0;
    return TRT_OK;
}

extern "C" int trt_read_counters(trt_context *ctx, unsigned long long *path_rays, unsigned long long *shadow_rays)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long c[kCounterSlots];
    HIP_TRY(hipMemcpy(c, ctx->d_counters.ptr, sizeof c, hipMemcpyDeviceToHost));
    ctx->last_trips = c[2];
    ctx->last_phase2 = c[3];
    ctx->last_swept = c[28];
    ctx->last_passes = c[29];
    for (int k = 0; k < 7; k++)
        ctx->last_loops[k] = c[30 + k];
#if defined(TRT_MARKS) && TRT_MARKS == 2
    if (getenv("TRT_PRINT_PROFILE"))
        for (int k = 0; k < trt::kProfileKinds; k++)
            for (int s = 0; s < 64; s++)
                if (c[trt::kProfileAt + 64 * k + s])
                    fprintf(stderr, "profile %d %d %llu\n", k, s, c[trt::kProfileAt + 64 * k + s]);
#endif
    if (path_rays)
        *path_rays = c[0];
    if (shadow_rays)
        *shadow_rays = c[1];
    return TRT_OK;
}

// ---- the launch of a frame, or of several cameras of one scene (on the host a single frame is a batch of one) ----

// What a launch leaves of a frame: the Screen's pixels of three doubles (TRT.c:188-193), the emitter's three bytes per pixel
// ((int)(c*255), TRT.c:1157-1163), the text the emitter makes of those bytes (TRT.c:1142-1172; trt_ansi.h), or the half-block text of
// them, two owned rows per line of text (trt_ansi_half.h), or those bytes as a kitty graphics-protocol image (trt_kitty.h), or either
// text in the xterm 256-colour palette (trt_ansi256.h, trt_ansi256_half.h).
enum Output : int { kDoubles, kBytes, kText, kHalfText, kKittyText, kText256, kHalfText256, kOutputs };

// What the launches, the checks and the host entries need of a kind, once: how long a frame of it is, the side no frame of it exceeds,
// where a host entry stages it and how it words its time; and of a text -- the kinds behind the ordered mean that are neither doubles
// nor bytes, which keep reduce_samples_kernel and reduce_samples_rgb8_kernel (launch_ordered_mean) -- the two kernels that write it, how
// many waves its lane map asks for, and the magics its kernels divide by (trt_text_map.h; trt_kitty.h has another lane map and no magics).
struct OutputKind
{
    unsigned long long (*bytes)(int width, long long rows); // of one frame of `rows` rows of `width` pixels
    int side_max;          // 0: any
    const char *too_large; // the refusal of a width or a row count above side_max
    int (*stage)(trt_context *ctx, size_t room, void **d_out); // the context's buffer with room for `room` bytes of it (render_host_as)
    const char *counted; // print_host_times(): what a host entry says it took its time for, and how many bytes one of them is
    size_t counted_bytes;
    trt::TextMeanKernel mean; // null: not a text
    trt::TextFromRgb8Kernel from_rgb8;
    unsigned long long (*waves)(unsigned long long address, unsigned long long bytes, bool several);
    unsigned (*row_magic)(int width), (*width_magic)(int width); // null: the kernels ignore the argument
};

static unsigned long long doubles_bytes(int width, long long rows) { return (unsigned long long)rows * width * 3 * sizeof(double); }
static unsigned long long rgb8_bytes(int width, long long rows) { return (unsigned long long)rows * width * 3; }

static int stage_in_framebuffer(trt_context *ctx, size_t room, void **d_out)
{
    HIP_TRY(ctx->d_fb.reserve((room + sizeof(double) - 1) / sizeof(double)));
    *d_out = ctx->d_fb.ptr;
    return TRT_OK;
}

template <DeviceBuffer<unsigned char> trt_context::*Buffer>
static int stage_in(trt_context *ctx, size_t room, void **d_out)
{
    HIP_TRY((ctx->*Buffer).reserve(room));
    *d_out = (ctx->*Buffer).ptr;
    return TRT_OK;
}

// A character-cell text's lane map, a wave per Kind().wave_words aligned words: ONE frame has exactly the waves its output address needs,
// the frames of several the most an alignment needs.  Its rows divide by their length.
template <trt_text_kind (*Kind)()>
static unsigned long long text_waves(unsigned long long address, unsigned long long bytes, bool several)
{
    return trt_text_waves(Kind(), several ? bytes / 4 : trt_text_split_of(address, bytes).words);
}

template <trt_text_kind (*Kind)()>
static unsigned text_row_magic(int width)
{
    return trt_text_magic((unsigned long long)trt_text_row_bytes(Kind(), width));
}

// the kitty image's: a wave per 64 word slots, the tail's among them
static unsigned long long kitty_waves(unsigned long long address, unsigned long long bytes, bool several)
{
    return several ? trt_kitty_waves_most(bytes) : trt_kitty_waves(address, bytes);
}

// a character-cell text's row: its Format (trt_ansi.hpp) for the kernels, its kind for the lane map and the rows' magic
template <class Format, trt_text_kind (*Kind)()>
static OutputKind character_cells(unsigned long long (*bytes)(int, long long), unsigned (*width_magic)(int))
{
    return {bytes, 0, nullptr, stage_in<&trt_context::d_text>, "bytes of text", 1, trt::reduce_samples_text_kernel<Format>, trt::text_from_rgb8_kernel<Format>,
            text_waves<Kind>, text_row_magic<Kind>, width_magic};
}

static const OutputKind kOutput[kOutputs] = {
    {doubles_bytes, 0, nullptr, stage_in_framebuffer, "bytes", 1},
    {rgb8_bytes, 0, nullptr, stage_in<&trt_context::d_rgb8>, "pixels", 3},
    character_cells<trt::ansi_text, trt_ansi_kind>(trt_ansi_text_bytes, nullptr),
    character_cells<trt::ansi_half_text, trt_ansi_half_kind>(trt_ansi_half_text_bytes, trt_ansi_half_width_magic),
    // five digits a side in the image's header
    {trt_kitty_text_bytes, TRT_KITTY_MAX, "a kitty image of %d x %d exceeds %d", stage_in<&trt_context::d_text>, "bytes of text", 1, trt::reduce_samples_kitty_kernel,
     trt::kitty_from_rgb8_kernel, kitty_waves, nullptr, nullptr},
    character_cells<trt::ansi256_text, trt_ansi256_kind>(trt_ansi256_text_bytes, nullptr),
    character_cells<trt::ansi256_half_text, trt_ansi256_half_kind>(trt_ansi256_half_text_bytes, trt_ansi256_half_width_magic),
};

static size_t frame_bytes(Output kind, int width, int rows) { return (size_t)kOutput[kind].bytes(width, rows); }

// the kind's side limit on a frame of width x rows: TRT_OK, or the refusal
static int check_side(Output kind, int width, int rows)
{
    const OutputKind &k = kOutput[kind];
    if (k.side_max && (width > k.side_max || rows > k.side_max))
        return fail(TRT_ERR_ARGUMENT, k.too_large, width, rows, k.side_max);
    return TRT_OK;
}

// what the device entries refuse, for `frames` cameras into one framebuffer of `frames` frames of the rowset
static int check_render_arguments(const trt_context *ctx, const Camera *cameras, int frames, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                  const void *d_pixels, size_t capacity_bytes, Output kind = kDoubles)
{
    if (!ctx || !cameras || !d_pixels)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (frames < 1 || frames > TRT_BATCH_MAX)
        return fail(TRT_ERR_ARGUMENT, "a batch has 1 to %d cameras, %d given", TRT_BATCH_MAX, frames);
    if (!rowset_valid(rows))
        return fail(TRT_ERR_ARGUMENT, "invalid rowset");
    if (bounce_limit < 1 || rays_per_pixel < 1) // bounce_limit 0 divides 0 by 0 in the reference (TRT.c:1061)
        return fail(TRT_ERR_ARGUMENT, "bounce_limit %d / rays_per_pixel %d", bounce_limit, rays_per_pixel);
    for (int b = 1; b < frames; b++) // the jitter and the screen axes are the batch's (main() moves only camera.frame, TRT.c:1327-1336)
        if (cameras[b].screen_width != cameras[0].screen_width || cameras[b].screen_height != cameras[0].screen_height ||
            cameras[b].screen_distance != cameras[0].screen_distance)
            return fail(TRT_ERR_ARGUMENT, "camera %d of the batch has another screen_width / screen_height / screen_distance than camera 0", b);
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "trt_set_scene has not been called");
    const int local_rows = trt_rowset_rows(rows);
    const int rc = check_side(kind, rows->width, local_rows);
    if (rc)
        return rc;
    const size_t need = frame_bytes(kind, rows->width, local_rows) * frames;
    if (capacity_bytes < need)
        return fail(TRT_ERR_CAPACITY, "framebuffer of %d frame(s) needs %zu B, %zu given", frames, need, capacity_bytes);
    if ((unsigned long long)local_rows * rows->width >= 0x7fffffffull)
        return fail(TRT_ERR_ARGUMENT, "%d x %d pixels exceed the 2^31 pixel index range", local_rows, rows->width);
    const unsigned long long units = (unsigned long long)local_rows * rows->width * rays_per_pixel * frames; // samples: the production kernel's work units
    if (ctx->kernel == 0 && units >= 0x7fffffffull)
        return fail(TRT_ERR_ARGUMENT, "%llu work units in %d frame(s) exceed the 2^31 index range", units, frames);
    return TRT_OK;
}

// min(ceil(2^32 / d), 2^32 - 1): x / d by multiply-high (trt_device.hpp, trt_rounds.hpp)
static unsigned division_magic(unsigned long long d)
{
    return (unsigned)std::min<unsigned long long>((0x100000000ull + d - 1) / d, 0xffffffffull);
}

// The frame view of `camera` over `rows` on lane set `lane_set`, but for what belongs to the launch (launch_render): the scratch, the
// image in device memory, the refraction indices, the rings' place and the queue's shape.
static trt::FrameView frame_view(const trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_pixels,
                                 int lane_set)
{
    trt::FrameView f{};
    memcpy(f.cam, camera, sizeof(Camera));
    f.jitter = ctx->d_jitter.ptr;
    f.col_x = ctx->d_axes.ptr;
    f.row_y = ctx->d_axes.ptr + rows->width;
    f.inv_spp = 1.0 / rays_per_pixel;
    f.width_magic = division_magic((unsigned)rows->width);
    f.spp_magic = division_magic((unsigned)rays_per_pixel);
    f.tile_magic = division_magic((unsigned)rows->tile_rows);
    f.out = (double *)d_pixels;
    f.counters = ctx->counters_enabled ? ctx->d_counters.ptr : nullptr;
#if defined(TRT_MARKS) && TRT_MARKS == 2
    f.counters = ctx->d_counters.ptr; // the ISA profile of the SHIPPING instantiations lands there
#endif
    f.queue = ctx->d_queue.ptr + trt::kQueueLaneWords * lane_set;
    f.width = rows->width;
    f.height = rows->height;
    f.tile_rows = rows->tile_rows;
    f.tile_first = rows->tile_first;
    f.tile_step = rows->tile_step;
    f.local_rows = trt_rowset_rows(rows);
    f.bounce_limit = bounce_limit;
    f.spp = rays_per_pixel;
    return f;
}

// The grid and the magics of one of a text's kernels over `frames` frames of width x rows at `out`: ONE frame's grid has exactly the waves
// its output address needs, that of several the most an alignment needs.
struct TextLaunch
{
    dim3 grid;
    unsigned row_magic, width_magic;
};

static TextLaunch text_launch(const OutputKind &k, const unsigned char *out, int width, int rows, unsigned frames)
{
    const unsigned long long waves = k.waves((unsigned long long)out, k.bytes(width, rows), frames > 1);
    return {dim3((unsigned)((waves * 64 + TRT_REDUCE_BLOCK - 1) / TRT_REDUCE_BLOCK), frames), k.row_magic ? k.row_magic(width) : 0u,
            k.width_magic ? k.width_magic(width) : 0u};
}

// the text of a frame that exists as RGB8 bytes: the formatting alone
static void launch_text_from_rgb8(hipStream_t stream, Output kind, const unsigned char *d_rgb8, int width, int rows, void *d_text)
{
    const TextLaunch t = text_launch(kOutput[kind], (const unsigned char *)d_text, width, rows, 1);
    hipLaunchKernelGGL(kOutput[kind].from_rgb8, t.grid, dim3(TRT_REDUCE_BLOCK), 0, stream, d_rgb8, (unsigned char *)d_text, width, rows, t.row_magic, t.width_magic);
}

// `lane_set` 0: the context's stream, queue word 0, d_samples; 1: the alternate stream, its own queue word and scratch
// (trt_render_host renders odd bands there).
// `entry`: a frame is one entry of the context's launch history (events, trt_kernel_times); the frames of a batch that is served
// one launch per camera are one entry together -- the first opens it (and clears the counters), the last closes it -- and so are
// the launches of a batch that was split for LDS.
enum : int { kEntryOpens = 1, kEntryCloses = 2, kEntryWhole = kEntryOpens | kEntryCloses };

// The reference-order kernel's launch: it has no scratch and no mean.  Its bytes are its doubles, rendered into the context's
// framebuffer, through quantize_kernel, and its text is those bytes through the kind's *_from_rgb8_kernel.
static int launch_reference(trt_context *ctx, const RenderPlan &plan, trt::FrameView f, void *out, Output kind, long pixels, hipStream_t stream, int entry)
{
    const int slot = (int)(ctx->launches % kEventRing);
    const bool text = kOutput[kind].from_rgb8 != nullptr;
    if (kind != kDoubles)
    {
        if (ctx->d_fb.capacity < (size_t)pixels * 3 || (text && ctx->d_text_rgb8.capacity < (size_t)pixels * 3))
            HIP_TRY(hipStreamSynchronize(stream)); // a frame in flight may still use the old framebuffer
        HIP_TRY(ctx->d_fb.reserve((size_t)pixels * 3));
        if (text) // text: the framebuffer's bytes first, in a buffer of the context's
            HIP_TRY(ctx->d_text_rgb8.reserve((size_t)pixels * 3));
        f.out = ctx->d_fb.ptr;
    }
    if (ctx->scratch_fill) // trt_set_scratch_fill: the reference-order kernel has no scratch
    {
        HIP_TRY(hipMemsetAsync(f.out, 0xFF, (size_t)pixels * 3 * sizeof(double), stream));
        if (kind != kDoubles)
            HIP_TRY(hipMemsetAsync(out, 0xFF, frame_bytes(kind, f.width, f.local_rows), stream));
    }
    if (entry & kEntryOpens)
        HIP_TRY(hipEventRecord(ctx->ev_start[slot], stream));
    const bool device_scene = plan.variant != kReference;
    const auto kernel = ctx->specular ? (device_scene ? trt::render_simple_kernel<true, true> : trt::render_simple_kernel<false, true>) // trt_set_specular
                      : ctx->sky_filter ? (device_scene ? trt::render_simple_kernel<true, false, true> : trt::render_simple_kernel<false, false, true>) // trt_set_sky_filter
                                        : (device_scene ? trt::render_simple_kernel<true> : trt::render_simple_kernel<false>);
    hipLaunchKernelGGL(kernel, dim3(plan.grid), dim3(plan.block), device_scene ? 0 : plan.lds, stream, ctx->scene, f);
    if (entry & kEntryCloses)
        HIP_TRY(hipEventRecord(ctx->ev_mid[slot], stream));
    if (kind != kDoubles)
        hipLaunchKernelGGL(trt::quantize_kernel, dim3((unsigned)((pixels * 3 + 255) / 256)), dim3(256), 0, stream, (const double *)f.out, pixels * 3,
                           text ? ctx->d_text_rgb8.ptr : (unsigned char *)out);
    if (text)
        launch_text_from_rgb8(stream, kind, ctx->d_text_rgb8.ptr, f.width, f.local_rows, out);
    if (entry & kEntryCloses)
        HIP_TRY(hipEventRecord(ctx->ev_stop[slot], stream));
    HIP_TRY(hipGetLastError());
    return TRT_OK;
}

// TRT.c:1063-1065: the mean over each pixel's samples, in sample order, of the `frames` frames of a launch whose scratch is `samples`,
// into `out` as `kind`: one kernel per kind, the frame in blockIdx.y.  It starts the queue for the next launch of this shape.  ONE
// frame's grid has exactly the lanes or waves its output address needs; the frames of several start at any alignment, so their grid is
// sized for the most an alignment needs (trt_common.hpp, trt_text_map.h).
static void launch_ordered_mean(hipStream_t stream, const RenderPlan &plan, const trt::FrameView &f, const double *samples, void *out, Output kind, long pixels,
                                unsigned frames)
{
    const long values = pixels * 3;
    const dim3 block(TRT_REDUCE_BLOCK);
    const auto blocks = [&](unsigned long long lanes) { return dim3((unsigned)((lanes + TRT_REDUCE_BLOCK - 1) / TRT_REDUCE_BLOCK), frames); };
    if (kind == kDoubles) // a lane per group of values and one per value the groups leave
        hipLaunchKernelGGL(trt::reduce_samples_kernel, blocks((unsigned long long)trt_mean_lanes(values)), block, 0, stream, samples, (double *)out, values, f.spp, f.inv_spp, f.queue, plan.grid,
                           plan.block / 64, f.queue_shift);
    else if (kind == kBytes) // a lane per group of four values and one per value of a frame's head and tail
        hipLaunchKernelGGL(trt::reduce_samples_rgb8_kernel,
                           blocks(frames > 1 ? values / trt::kRgb8Group + 6 : trt::rgb8_lanes(values, trt::rgb8_head((const unsigned char *)out, values))), block, 0,
                           stream, samples, (unsigned char *)out, values, f.spp, f.inv_spp, f.queue, plan.grid, plan.block / 64, f.queue_shift);
    else // a text: the waves its lane map asks for
    {
        const TextLaunch t = text_launch(kOutput[kind], (const unsigned char *)out, f.width, f.local_rows, frames);
        hipLaunchKernelGGL(kOutput[kind].mean, t.grid, block, 0, stream, samples, (unsigned char *)out, f.width, f.local_rows, t.row_magic, t.width_magic, f.spp, f.inv_spp,
                           f.queue, plan.grid, plan.block / 64, f.queue_shift);
    }
}

// The production kernel's launch (kernel 0): the queue started unless the launch before left it ready, the image staged for the
// DEVICE_IMAGE instantiations, persistent waves in synchronous rounds over SAMPLE units -- over the frame `f`, or with `batch` the plan's
// BATCH form over the frames of `batch`, of which f is the first -- then the ordered mean of every frame's `pixels` pixels into `out`.
static int launch_production(trt_context *ctx, const RenderPlan &plan, trt::FrameView f, const trt::GridView &grids, const trt::BatchView *batch, void *out,
                             Output kind, long pixels, int lane_set, int entry)
{
    const hipStream_t stream = lane_set ? ctx->alt_stream : ctx->stream;
    const int slot = (int)(ctx->launches % kEventRing);
    const dim3 grid(plan.grid), block(plan.block);
    unsigned *const ready = ctx->queue_ready[lane_set];
    const RoundsVariant &k = kRounds[plan.variant];
    const unsigned frames = batch ? batch->frames : 1u;
    // scratch [frame][k][pixel][3]; the launches of a split batch follow one another on the stream
    DeviceBuffer<double> &scratch = lane_set ? ctx->d_samples_alt : ctx->d_samples;
    const size_t samples = (size_t)pixels * f.spp * frames * 3;
    if (scratch.capacity < samples)
        HIP_TRY(hipStreamSynchronize(stream)); // a frame in flight may still use the old scratch
    HIP_TRY(scratch.reserve(samples));
    f.samples = scratch.ptr;
    if (k.image)
    { // a buffer per lane set: trt_render_host renders bands on two streams at once
        DeviceBuffer<double> &image = lane_set ? ctx->d_image_alt : ctx->d_image;
        const size_t doubles = image_lds_bytes(ctx, f.spp) / sizeof(double);
        if (image.capacity < doubles)
            HIP_TRY(hipStreamSynchronize(stream)); // a frame in flight may still read the old image
        HIP_TRY(image.reserve(doubles));
        f.image = image.ptr;
    }
    if (ctx->ior_count && ctx->ior_count != ctx->scene.num_spheres) // before the first event of the launch is recorded
        return fail(TRT_ERR_ARGUMENT, "trt_set_refraction was given %d indices, the scene has %d spheres", ctx->ior_count, ctx->scene.num_spheres);
    if (ctx->ior_count)
        f.ior = ctx->d_ior.ptr;
    f.ring_at = plan.ring_at;
    f.queue_shift = plan.queue_shift;
    f.chunk = plan.chunk;
    if (ctx->scratch_fill)
    { // trt_set_scratch_fill: exactly the launch's samples and exactly its pixels read as NaN until the launch writes them
        HIP_TRY(hipMemsetAsync(scratch.ptr, 0xFF, samples * sizeof(double), stream));
        HIP_TRY(hipMemsetAsync(out, 0xFF, frame_bytes(kind, f.width, f.local_rows) * frames, stream));
    }
    const bool left_ready = ready[0] == plan.grid && ready[1] == plan.block / 64 && ready[2] == f.queue_shift; // by the frame before
    ready[0] = 0; // the render kernel uses it up; ready again once this frame's launches have gone in
    if (!left_ready)
        hipLaunchKernelGGL(trt::start_queue_kernel, dim3(1), dim3(64), 0, stream, f.queue, plan.grid, plan.block / 64, f.queue_shift);
    if (entry & kEntryOpens)
        HIP_TRY(hipEventRecord(ctx->ev_start[slot], stream));
    if (k.image)
        hipLaunchKernelGGL(stage_image_kernel, dim3(1), dim3(kImageBlock), 0, stream, ctx->scene, ctx->cull, f, grids);
    if (batch)
        hipLaunchKernelGGL(k.batch, grid, block, plan.lds, stream, ctx->scene, ctx->cull, f, grids, *batch);
    else
        hipLaunchKernelGGL(k.fn, grid, block, plan.lds, stream, ctx->scene, ctx->cull, f, grids);
    if (entry & kEntryCloses)
        HIP_TRY(hipEventRecord(ctx->ev_mid[slot], stream)); // of a split batch: the last launch's
#if !TRT_AB_SKIP_REDUCE // diagnostic build (profiles/r03: what the ordered mean's streaming pass costs in the pipelined loop)
    launch_ordered_mean(stream, plan, f, scratch.ptr, out, kind, pixels, frames);
#endif
    if (entry & kEntryCloses)
        HIP_TRY(hipEventRecord(ctx->ev_stop[slot], stream));
    HIP_TRY(hipGetLastError());
#if !TRT_AB_SKIP_REDUCE
    ready[0] = plan.grid, ready[1] = plan.block / 64, ready[2] = f.queue_shift; // what the ordered mean left the queue ready for
#endif
    return TRT_OK;
}

// Carries out a planned launch on the route its variant takes, into `out` as `kind`: doubles, (kBytes) cast to the emitter's bytes in
// the ordered mean's pass, or (the texts) cast and formatted as the terminal's text in the same pass.
static int launch_render(trt_context *ctx, const RenderPlan &plan, const trt::FrameView &f, const trt::GridView &grids, const trt::BatchView *batch, void *out,
                         Output kind, long pixels, int lane_set, int entry)
{
    const hipStream_t stream = lane_set ? ctx->alt_stream : ctx->stream;
    const bool reference = plan.variant == kReference || plan.variant == kReferenceImage;
    if (ctx->ior_count && ctx->specular) // whichever kernel: nothing of the launch has been recorded yet, the context renders again once one is off
        return fail(TRT_ERR_ARGUMENT, "the refraction extension (trt_set_refraction) and the specular extension (trt_set_specular) do not combine yet");
    if (ctx->sky_filter && (ctx->ior_count || ctx->specular)) // the same
        return fail(TRT_ERR_ARGUMENT, "bilinear sky filtering (trt_set_sky_filter) and the %s do not combine yet",
                    ctx->ior_count ? "refraction extension (trt_set_refraction)" : "specular extension (trt_set_specular)");
    if (ctx->sky_filter && ctx->scene_image == 1 && !reference) // the caller asks for the device image, which the filter's instantiations do not have
        return fail(TRT_ERR_CAPACITY, "bilinear sky filtering stages the scene image in LDS only: trt_set_scene_image(ctx, 1) cannot be served");
    if (plan.lds > (size_t)ctx->lds_limit) // LDS only (trt_set_scene_image(ctx, 0)), or an extension, neither of which has a device-image form
        return fail(TRT_ERR_CAPACITY, "%s and %d rays per pixel need %zu B of LDS staging, device offers %d%s", plan.variant == kReference ? "scene" : "scene image",
                    f.spp, plan.lds, ctx->lds_limit,
                    plan.variant == kReference ? "" : ctx->ior_count ? " (the refraction extension stages it in LDS only)"
                    : ctx->specular            ? " (the specular extension stages it in LDS only)"
                    : ctx->sky_filter          ? " (bilinear sky filtering stages it in LDS only)" : "");
#if defined(TRT_MARKS) && TRT_MARKS == 2
    HIP_TRY(hipMemsetAsync(ctx->d_counters.ptr, 0, kCounterSlots * sizeof(unsigned long long), stream));
#endif
    const int rc = reference ? launch_reference(ctx, plan, f, out, kind, pixels, stream, entry)
                             : launch_production(ctx, plan, f, grids, batch, out, kind, pixels, lane_set, entry);
    if (rc)
        return rc;
    ctx->last_variant = plan.variant;
    ctx->last_spp = f.spp;
    if (entry & kEntryCloses)
        ctx->launches++;
    return TRT_OK;
}

static int render_device_on(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_pixels,
                            size_t capacity_bytes, int lane_set, int entry = kEntryWhole, Output kind = kDoubles)
{
    int rc = check_render_arguments(ctx, camera, 1, rows, bounce_limit, rays_per_pixel, d_pixels, capacity_bytes, kind);
    if (rc)
        return rc;
    const long pixels = (long)trt_rowset_rows(rows) * rows->width;
    if (pixels == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t stream = lane_set ? ctx->alt_stream : ctx->stream;
    rc = prepare_jitter(ctx, camera, rows->width, rows->height, rays_per_pixel);
    if (rc)
        return rc;
    rc = prepare_axes(ctx, camera, rows->width, rows->height);
    if (rc)
        return rc;
    rc = ensure_eye_tables(ctx, camera, stream); // no-op unless the eye moved (trt_render_host builds them before it forks its streams)
    if (rc)
        return rc;
    if (ctx->counters_enabled && (entry & kEntryOpens))
        HIP_TRY(hipMemsetAsync(ctx->d_counters.ptr, 0, kCounterSlots * sizeof(unsigned long long), stream));
    RenderPlan plan;
    rc = plan_render(ctx, pixels * rays_per_pixel, rays_per_pixel, 1, false, &plan);
    if (rc)
        return rc;
    // only the reference-order kernel writes FrameView::out: doubles (launch_reference gives it the context's framebuffer when bytes or text are asked for)
    return launch_render(ctx, plan, frame_view(ctx, camera, rows, bounce_limit, rays_per_pixel, kind == kDoubles ? d_pixels : nullptr, lane_set), ctx->grids, nullptr,
                         d_pixels, kind, pixels, lane_set, entry);
}

extern "C" int trt_render_device(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                                 int rays_per_pixel, void *d_pixels, size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_pixels, capacity_bytes, 0);
}

extern "C" int trt_render_device_rgb8(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_rgb8,
                                      size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_rgb8, capacity_bytes, 0, kEntryWhole, kBytes);
}

extern "C" size_t trt_ansi_bytes(int width, int rows)
{
    return (size_t)trt_ansi_text_bytes(width, rows);
}

extern "C" int trt_render_device_ansi(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                      size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, 0, kEntryWhole, kText);
}

extern "C" size_t trt_ansi_half_bytes(int width, int rows)
{
    return (size_t)trt_ansi_half_text_bytes(width, rows);
}

extern "C" int trt_render_device_ansi_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                           size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, 0, kEntryWhole, kHalfText);
}

static int text_from_rgb8_device(trt_context *ctx, Output kind, const void *d_rgb8, int width, int rows, void *d_text)
{
    if (!ctx || !d_rgb8 || !d_text)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (width <= 0 || rows <= 0 || (unsigned long long)width * rows >= 0x7fffffffull)
        return fail(TRT_ERR_ARGUMENT, "screen %d x %d", width, rows);
    HIP_TRY(hipSetDevice(ctx->device));
    launch_text_from_rgb8(ctx->stream, kind, (const unsigned char *)d_rgb8, width, rows, d_text);
    HIP_TRY(hipGetLastError());
    return TRT_OK;
}

extern "C" int trt_ansi_half_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text)
{
    return text_from_rgb8_device(ctx, kHalfText, d_rgb8, width, rows, d_text);
}

extern "C" int trt_ansi_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text)
{
    return text_from_rgb8_device(ctx, kText, d_rgb8, width, rows, d_text);
}

extern "C" size_t trt_kitty_bytes(int width, int rows)
{
    return (size_t)trt_kitty_text_bytes(width, rows);
}

extern "C" int trt_render_device_kitty(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                       size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, 0, kEntryWhole, kKittyText);
}

extern "C" int trt_kitty_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text)
{
    const int rc = check_side(kKittyText, width, rows);
    return rc ? rc : text_from_rgb8_device(ctx, kKittyText, d_rgb8, width, rows, d_text);
}

extern "C" size_t trt_ansi256_bytes(int width, int rows)
{
    return (size_t)trt_ansi256_text_bytes(width, rows);
}

extern "C" size_t trt_ansi256_half_bytes(int width, int rows)
{
    return (size_t)trt_ansi256_half_text_bytes(width, rows);
}

extern "C" int trt_render_device_ansi256(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                         size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, 0, kEntryWhole, kText256);
}

extern "C" int trt_render_device_ansi256_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                              size_t capacity_bytes)
{
    return render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, 0, kEntryWhole, kHalfText256);
}

extern "C" int trt_ansi256_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text)
{
    return text_from_rgb8_device(ctx, kText256, d_rgb8, width, rows, d_text);
}

extern "C" int trt_ansi256_half_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text)
{
    return text_from_rgb8_device(ctx, kHalfText256, d_rgb8, width, rows, d_text);
}

extern "C" int trt_xterm256_from_rgb8_device(trt_context *ctx, const void *d_rgb8, size_t num_pixels, void *d_index)
{
    if (!ctx || !d_rgb8 || !d_index)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (num_pixels == 0)
        return TRT_OK;
    if (num_pixels > 0x7fffffffull * 256) // a lane a pixel, 256 a block
        return fail(TRT_ERR_ARGUMENT, "%zu pixels exceed one launch", num_pixels);
    HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(trt::xterm256_from_rgb8_kernel, dim3((unsigned)((num_pixels + 255) / 256)), dim3(256), 0, ctx->stream, (const unsigned char *)d_rgb8,
                       (unsigned char *)d_index, (unsigned long long)num_pixels);
    HIP_TRY(hipGetLastError());
    return TRT_OK;
}

extern "C" int trt_quantize_device(trt_context *ctx, const void *d_pixels, size_t num_pixels, void *d_rgb8)
{
    if (!ctx || !d_pixels || !d_rgb8)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (num_pixels == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const long n = (long)num_pixels * 3;
    hipLaunchKernelGGL(trt::quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)d_pixels,
                       n, (unsigned char *)d_rgb8);
    HIP_TRY(hipGetLastError());
    return TRT_OK;
}

extern "C" int trt_synchronize(trt_context *ctx)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return TRT_OK;
}

extern "C" int trt_render_host(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                               int rays_per_pixel, Vector *pixels)
{
    if (!ctx || !pixels)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!rowset_valid(rows))
        return fail(TRT_ERR_ARGUMENT, "invalid rowset");
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t count = (size_t)trt_rowset_rows(rows) * rows->width;
    const size_t bytes = count * sizeof(Vector);
    HIP_TRY(ctx->d_fb.reserve(count * 3));
    HIP_TRY(ctx->h_staging.reserve(bytes));
    const double t_begin = host_now_ms();
    // A whole frame is rendered in up to four bands of rows: while band b+1 is being rendered, band b crosses PCIe on the
    // copy stream into pinned staging, chunk by chunk (an event per chunk), and a few host threads copy landed chunks
    // into the caller's (pageable) buffer.  Shards and small frames are one band.
    const int local_rows = trt_rowset_rows(rows);
    const bool whole = rows->tile_first == 0 && rows->tile_step == 1 && rows->tile_rows >= rows->height;
    static const int band_count = getenv("TRT_HOST_BANDS") ? std::min(8, std::max(1, atoi(getenv("TRT_HOST_BANDS")))) : 4;
#if defined(TRT_MARKS) && TRT_MARKS == 2
    const int bands = 1; // the ISA profile is of ONE launch
#else
    const int bands = whole && !ctx->counters_enabled && local_rows >= 256 && bytes >= (32u << 20) ? band_count : 1;
#endif
    const int band_rows = (local_rows + bands - 1) / bands;
    const size_t row_bytes = (size_t)rows->width * sizeof(Vector);
    const int chunks_per_band = (int)std::min<size_t>(16 / bands, std::max<size_t>(1, (size_t)band_rows * row_bytes / (4u << 20)));
    int chunks = 0;
    size_t chunk_at[16], chunk_len[16];
    if (bands > 1 && !ctx->copy_stream)
    { // created on first use: every stream of a process competes for a handful of hardware queues, and two streams that
      // land on one queue run one after the other (a renderer that never comes here keeps its streams to itself)
        HIP_TRY(ctx->copy_stream.create());
        HIP_TRY(ctx->alt_stream.create());
    }
    const hipStream_t copy_stream = bands > 1 ? ctx->copy_stream : ctx->stream;
    if (ctx->have_scene && camera)
    { // both render streams read the eye's tables: build them before the fork
        const int rc = ensure_eye_tables(ctx, camera, ctx->stream);
        if (rc)
            return rc;
    }
    if (bands > 1)
    { // the alternate stream starts behind whatever the caller queued on the context's stream before this call
        HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->alt_stream, ctx->ev_fork, 0));
    }
    for (int b = 0; b < bands; b++)
    {
        trt_rowset band = *rows;
        if (bands > 1)
            band = trt_rowset{rows->width, rows->height, band_rows, b, bands};
        const int rows_here = trt_rowset_rows(&band);
        const size_t at = (size_t)b * band_rows * row_bytes, len = (size_t)rows_here * row_bytes;
        const int set = bands > 1 ? (b & 1) : 0; // odd bands on the alternate stream: a band's tail and reduction overlap the next band
        int rc = render_device_on(ctx, camera, &band, bounce_limit, rays_per_pixel, (char *)ctx->d_fb.ptr + at, len, set);
        if (rc)
            return rc;
        if (bands > 1)
        { // a second stream costs ~0.1 ms of cross-queue hand-over: only where there is something to overlap
            HIP_TRY(hipEventRecord(ctx->ev_band[b], set ? ctx->alt_stream : ctx->stream));
            HIP_TRY(hipStreamWaitEvent(copy_stream, ctx->ev_band[b], 0));
        }
        const size_t per = ((len + chunks_per_band - 1) / chunks_per_band + 63) / 64 * 64;
        for (int i = 0; i < chunks_per_band; i++, chunks++)
        {
            chunk_at[chunks] = at + (size_t)i * per;
            chunk_len[chunks] = (size_t)i * per < len ? std::min(per, len - (size_t)i * per) : 0;
            if (chunk_len[chunks])
                HIP_TRY(hipMemcpyAsync((char *)ctx->h_staging.ptr + chunk_at[chunks], (const char *)ctx->d_fb.ptr + chunk_at[chunks], chunk_len[chunks],
                                       hipMemcpyDeviceToHost, copy_stream));
            HIP_TRY(hipEventRecord(ctx->ev_chunk[chunks], copy_stream));
        }
    }
    const double t_enqueued = host_now_ms();
    const int workers = chunks >= 4 ? 4 : 1;
    hipError_t worker_error[4] = {hipSuccess, hipSuccess, hipSuccess, hipSuccess};
    auto drain = [&](int w) {
        (void)hipSetDevice(ctx->device);
        for (int i = w; i < chunks; i += workers)
        {
            const hipError_t e = hipEventSynchronize(ctx->ev_chunk[i]);
            if (e != hipSuccess)
            {
                worker_error[w] = e;
                return;
            }
            memcpy((char *)pixels + chunk_at[i], (const char *)ctx->h_staging.ptr + chunk_at[i], chunk_len[i]);
        }
    };
    if (workers == 1)
        drain(0);
    else
    {
        std::thread pool[3];
        for (int w = 1; w < workers; w++)
            pool[w - 1] = std::thread(drain, w);
        drain(0);
        for (int w = 1; w < workers; w++)
            pool[w - 1].join();
    }
    for (int w = 0; w < workers; w++)
        HIP_TRY(worker_error[w]);
    if (bands > 1)
    {
        HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
        HIP_TRY(hipStreamSynchronize(ctx->alt_stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (print_host_times())
        fprintf(stderr, "trt_render_host: %d band(s), enqueue %.3f ms, render + copy-out of %zu bytes %.3f ms\n", bands, t_enqueued - t_begin, bytes,
                host_now_ms() - t_enqueued);
    return TRT_OK;
}

// ---- several cameras per call ----

// How many of the next `remaining` frames go into ONE launch, and its plan: the most whose larger image costs no resident
// workgroup against the image of one frame (a batch of one always goes).  Negative: an error.
static int fit_batch(trt_context *ctx, long units_per_frame, int spp, int remaining, RenderPlan *plan)
{
    for (int t = remaining;; t--)
    {
        int rc = plan_render(ctx, units_per_frame * t, spp, t, true, plan), alone = 0;
        if (!rc)
            rc = blocks_per_cu(ctx, plan->variant, true, launch_lds_bytes(ctx, plan->variant, spp), &alone);
        if (rc)
            return rc;
        if (t == 1 || (plan->per_cu > 0 && plan->per_cu >= alone))
            return t;
    }
}

// a batch of more than one camera builds its eye tables in the slots of the context's own tables: shared tables have none to spare
static int check_batch_tables(const trt_context *ctx, int n)
{
    if (n > 1 && ctx->T.use_count() > 1)
        return fail(TRT_ERR_CAPACITY, "this context's scene tables are shared with %ld other context(s) (trt_share_scene): their eye slots are the sharers', "
                                      "a batch of %d cameras has none to build its tables in (one camera per call works)", ctx->T.use_count() - 1, n);
    return TRT_OK;
}

// frame b in `kind` at d_pixels + b * frame_bytes(kind, width, owned rows)
static int render_device_batch(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_pixels,
                               size_t capacity_bytes, Output kind)
{
    int rc = check_render_arguments(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_pixels, capacity_bytes, kind);
    if (rc)
        return rc;
    const long pixels = (long)trt_rowset_rows(rows) * rows->width, units = pixels * rays_per_pixel;
    const size_t each = frame_bytes(kind, rows->width, trt_rowset_rows(rows));
    const bool shared = ctx->T.use_count() > 1;
    rc = check_batch_tables(ctx, n);
    if (rc)
        return rc;
    ctx->batch_frames = n;
    ctx->batch_launches = 0;
    if (pixels == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t stream = ctx->stream;
    // everything without a BATCH form -- and a bounce limit that leaves no room for the frame beside the bounce count -- one launch per camera
    if (shared || bounce_limit > trt::kBatchBounceMask || !batch_form(choose_variant(ctx, units * n, rays_per_pixel, n)))
    {
        for (int b = 0; b < n; b++)
        {
            rc = render_device_on(ctx, &cameras[b], rows, bounce_limit, rays_per_pixel, (char *)d_pixels + (size_t)b * each, each, 0, (b == 0 ? kEntryOpens : 0) | (b == n - 1 ? kEntryCloses : 0), kind);
            if (rc)
                return rc;
            ctx->batch_launches++;
        }
        return TRT_OK;
    }
    rc = prepare_jitter(ctx, &cameras[0], rows->width, rows->height, rays_per_pixel);
    if (rc)
        return rc;
    rc = prepare_axes(ctx, &cameras[0], rows->width, rows->height);
    if (rc)
        return rc;
    for (int b = 0; b < n; b++) // frame b's eye tables in eye slot b of the context's own tables
    {
        rc = ensure_eye_tables(ctx, &cameras[b], stream, b);
        if (rc)
            return rc;
    }
    RenderPlan plan;
    int m = n;
    for (int first = 0; first < n; first += m)
    {
        m = fit_batch(ctx, units, rays_per_pixel, std::min(m, n - first), &plan);
        if (m < 0)
            return m;
        trt::GridView g = ctx->grids; // frame b of the launch: eye slot first + b
        g.eye_at = (unsigned)((size_t)first * 2 * 6 * (size_t)g.g_eye * (size_t)g.g_eye);
        trt::BatchView batch{};
        for (int b = 0; b < m; b++)
        {
            memcpy(batch.cam[b], &cameras[first + b], sizeof(Camera));
            batch.eye[b][0] = ctx->eye_slots[first + b].families[0], batch.eye[b][1] = ctx->eye_slots[first + b].families[1];
        }
        g.eye[0] = batch.eye[0][0], g.eye[1] = batch.eye[0][1];
        batch.frames = (unsigned)m;
        batch.units_per_frame = (unsigned)units;
        batch.frame_magic = division_magic((unsigned long long)units);
        rc = launch_render(ctx, plan, frame_view(ctx, &cameras[first], rows, bounce_limit, rays_per_pixel, kind == kDoubles ? d_pixels : nullptr, 0), g, &batch,
                           (char *)d_pixels + (size_t)first * each, kind, pixels, 0,
                           (first == 0 ? kEntryOpens : 0) | (first + m == n ? kEntryCloses : 0));
        if (rc)
            return rc;
        ctx->batch_launches++;
    }
    return TRT_OK;
}

extern "C" int trt_render_device_batch(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                       void *d_pixels, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_pixels, capacity_bytes, kDoubles);
}

extern "C" int trt_render_device_batch_rgb8(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                            void *d_rgb8, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_rgb8, capacity_bytes, kBytes);
}

extern "C" int trt_render_device_batch_ansi(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                            void *d_text, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, kText);
}

// The copy-out of the host entries: `n` cameras rendered as `kind` into the context's buffer of that kind, copied to pinned staging
// and, the stream synchronised, to the caller's `host`.  The ordered mean writes the bytes ((int)(c*255), TRT.c:1157-1163) and the text
// (TRT.c:1142-1172) itself: no framebuffer of doubles on the way, and no formatting on the host.  `batch`: the batch route, which picks
// the render kernel's BATCH form and counts for trt_batch_info; otherwise the single frame's, timed as `name` under print_host_times().
static int render_host_as(trt_context *ctx, const Camera *cameras, int n, bool batch, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *host,
                          Output kind, const char *name = nullptr)
{
    if (!ctx || !host)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (batch && (n < 1 || n > TRT_BATCH_MAX))
        return fail(TRT_ERR_ARGUMENT, "a batch has 1 to %d cameras, %d given", TRT_BATCH_MAX, n);
    if (!rowset_valid(rows))
        return fail(TRT_ERR_ARGUMENT, "invalid rowset");
    HIP_TRY(hipSetDevice(ctx->device));
    int rc = check_side(kind, rows->width, trt_rowset_rows(rows));
    if (rc)
        return rc;
    const size_t bytes = (size_t)n * frame_bytes(kind, rows->width, trt_rowset_rows(rows));
    if (!batch && bytes == 0)
        return TRT_OK;
    const size_t room = std::max<size_t>(bytes, 1);
    void *d_out;
    rc = kOutput[kind].stage(ctx, room, &d_out);
    if (rc)
        return rc;
    HIP_TRY(ctx->h_staging.reserve(room));
    const double t_begin = host_now_ms();
    rc = batch ? render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_out, bytes, kind)
               : render_device_on(ctx, cameras, rows, bounce_limit, rays_per_pixel, d_out, bytes, 0, kEntryWhole, kind);
    if (rc || bytes == 0)
        return rc;
    HIP_TRY(hipMemcpyAsync(ctx->h_staging.ptr, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(host, ctx->h_staging.ptr, bytes);
    if (name && print_host_times())
        fprintf(stderr, "%s: %.3f ms for %zu %s\n", name, host_now_ms() - t_begin, bytes / kOutput[kind].counted_bytes, kOutput[kind].counted);
    return TRT_OK;
}

extern "C" int trt_render_host_rgb8(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                    unsigned char *rgb)
{
    return render_host_as(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, rgb, kBytes, "trt_render_host_rgb8");
}

extern "C" int trt_render_host_ansi(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, kText, "trt_render_host_ansi");
}

extern "C" int trt_render_host_batch(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                     Vector *pixels)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, pixels, kDoubles);
}

extern "C" int trt_render_host_batch_rgb8(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                          unsigned char *rgb)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, rgb, kBytes);
}

extern "C" int trt_render_host_batch_ansi(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, kText);
}

extern "C" int trt_render_device_batch_ansi_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                                 void *d_text, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, kHalfText);
}

extern "C" int trt_render_host_ansi_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, kHalfText, "trt_render_host_ansi_half");
}

extern "C" int trt_render_host_batch_ansi_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                               char *text)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, kHalfText);
}

extern "C" int trt_render_device_batch_kitty(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                             void *d_text, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, kKittyText);
}

extern "C" int trt_render_host_kitty(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, kKittyText, "trt_render_host_kitty");
}

extern "C" int trt_render_host_batch_kitty(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, kKittyText);
}

extern "C" int trt_render_host_ansi256(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, kText256, "trt_render_host_ansi256");
}

extern "C" int trt_render_host_ansi256_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, kHalfText256, "trt_render_host_ansi256_half");
}

extern "C" int trt_render_device_batch_ansi256(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                               void *d_text, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, kText256);
}

extern "C" int trt_render_device_batch_ansi256_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                                    void *d_text, size_t capacity_bytes)
{
    return render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, kHalfText256);
}

extern "C" int trt_render_host_batch_ansi256(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, kText256);
}

extern "C" int trt_render_host_batch_ansi256_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                                  char *text)
{
    return render_host_as(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, kHalfText256);
}

extern "C" int trt_batch_info(trt_context *ctx, int *frames, int *render_launches)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    if (frames)
        *frames = ctx->batch_frames;
    if (render_launches)
        *render_launches = ctx->batch_launches;
    return TRT_OK;
}

// The event slots of the context's last launches, at most `max` and oldest first, the stream synchronised: each(i, slot), which
// returns an error or TRT_OK.  Returns how many launches there were, or the error.
template <class Each>
static int for_last_launches(trt_context *ctx, int max, Each each)
{
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const long n = std::min<long>(std::min<long>(ctx->launches, kEventRing), max);
    for (long i = 0; i < n; i++)
    {
        const int rc = each(i, (int)((ctx->launches - n + i) % kEventRing));
        if (rc)
            return rc;
    }
    return (int)n;
}

extern "C" int trt_kernel_times(trt_context *ctx, float *ms, int max)
{
    if (!ctx || !ms || max < 0)
        return fail(TRT_ERR_ARGUMENT, "bad argument");
    return for_last_launches(ctx, max, [&](long i, int slot) -> int {
        HIP_TRY(hipEventElapsedTime(&ms[i], ctx->ev_start[slot], ctx->ev_stop[slot]));
        return TRT_OK;
    });
}

extern "C" int trt_render_kernel_times(trt_context *ctx, float *render_ms, float *reduce_ms, int max)
{
    if (!ctx || !render_ms || max < 0)
        return fail(TRT_ERR_ARGUMENT, "bad argument");
    return for_last_launches(ctx, max, [&](long i, int slot) -> int {
        HIP_TRY(hipEventElapsedTime(&render_ms[i], ctx->ev_start[slot], ctx->ev_mid[slot]));
        if (reduce_ms)
            HIP_TRY(hipEventElapsedTime(&reduce_ms[i], ctx->ev_mid[slot], ctx->ev_stop[slot]));
        return TRT_OK;
    });
}

// trt_hip_diag.h: how many frames the context has launched, and the device time from the START of launch `first_launch` of context
// `first` to the END (render kernel and ordered mean) of launch `last_launch` of context `last` -- the span of a pipelined loop
// whose frames take turns over several contexts.  Launch numbers count from 0; the contexts keep the events of their last 256.
extern "C" long trt_launch_count(trt_context *ctx) { return ctx ? ctx->launches : -1; }

extern "C" int trt_launch_span_ms(trt_context *first, long first_launch, trt_context *last, long last_launch, float *ms)
{
    if (!first || !last || !ms || first->device != last->device)
        return fail(TRT_ERR_ARGUMENT, "bad argument");
    if (first_launch < 0 || first_launch >= first->launches || first->launches - first_launch > kEventRing || last_launch < 0 ||
        last_launch >= last->launches || last->launches - last_launch > kEventRing)
        return fail(TRT_ERR_ARGUMENT, "launches %ld / %ld are not among the last %d of their contexts (%ld / %ld launched)", first_launch, last_launch,
                    kEventRing, first->launches, last->launches);
    HIP_TRY(hipSetDevice(first->device));
    HIP_TRY(hipStreamSynchronize(first->stream));
    HIP_TRY(hipStreamSynchronize(last->stream));
    HIP_TRY(hipEventElapsedTime(ms, first->ev_start[first_launch % kEventRing], last->ev_stop[last_launch % kEventRing]));
    return TRT_OK;
}

extern "C" int trt_render_variant(trt_context *ctx, int *decoupled, int *workgroup_threads)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    const Variant v = described_variant(ctx);
    if (decoupled)
        *decoupled = v < kReference && kRounds[v].rings ? 1 : 0;
    if (workgroup_threads)
        *workgroup_threads = v >= kReference ? 256 : kRounds[v].block;
    return TRT_OK;
}

extern "C" int trt_set_scene_image(trt_context *ctx, int mode)
{
    if (!ctx || mode < -1 || mode > 1)
        return fail(TRT_ERR_ARGUMENT, "scene image mode %d", mode);
    ctx->scene_image = mode;
    // LDS only on a scene that does not fit: its frames fail (render_device_on), as trt_set_scene would have
    return ctx->have_scene && mode != 0 ? refresh_occupancy(ctx) : TRT_OK;
}

extern "C" int trt_render_image(trt_context *ctx, int *in_device_memory, unsigned long long *image_bytes)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    const Variant v = described_variant(ctx);
    if (in_device_memory)
        *in_device_memory = image_in_device_memory(v) ? 1 : 0;
    if (image_bytes)
        *image_bytes = !ctx->have_scene ? 0ull : v >= kReference ? scene_lds_bytes(ctx->scene) : image_lds_bytes(ctx, described_spp(ctx));
    return TRT_OK;
}

extern "C" int trt_kernel_info(trt_context *ctx, int *vgprs, int *sgprs, int *static_lds_bytes, int *max_blocks_per_cu,
                               int *compute_units)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    const Variant v = described_variant(ctx);
    hipFuncAttributes attr;
    HIP_TRY(hipFuncGetAttributes(&attr, v == kReference ? (const void *)trt::render_simple_kernel<false>
                                      : v == kReferenceImage ? (const void *)trt::render_simple_kernel<true> : (const void *)kRounds[v].fn));
    if (vgprs)
        *vgprs = attr.numRegs;
    if (sgprs)
        *sgprs = 0; // not reported by hipFuncGetAttributes; see profiles/*resource_usage*.txt
    if (static_lds_bytes)
        *static_lds_bytes = (int)attr.sharedSizeBytes;
    if (max_blocks_per_cu)
    { // what the launch is sized by: the 256-thread variants by the plain instantiation's occupancy
        int blocks = 0;
        if (v == kReference)
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, trt::render_simple_kernel<false>, 256, ctx->have_scene ? scene_lds_bytes(ctx->scene) : 0));
        else if (v == kReferenceImage)
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, trt::render_simple_kernel<true>, 256, 0));
        else if (!ctx->have_scene) // nothing stored yet: the plain instantiation without an image
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kRounds[kPlain].fn, trt::kPersistentBlock, 0));
        else
            (void)blocks_per_cu(ctx, v, false, 0, &blocks);
        *max_blocks_per_cu = blocks;
    }
    if (compute_units)
        *compute_units = ctx->compute_units;
    return TRT_OK;
}

// ---- the delta texts (trt_ansi_delta.h: the full text's cells; trt_ansi_delta_half.h: half-block cells; trt_ansi256_delta.h and
// trt_ansi256_delta_half.h: the two in the xterm 256-colour palette; trt_ansi_delta_chain.h: a chain of n texts; trt_ansi_delta.hpp: the
// kernels).  ONE path for the four KINDS (DeltaKind): the text between two frames is a chain of one, a single frame a batch of one ----

static_assert(TRT_DELTA_CHAIN_MAX == TRT_BATCH_MAX, "a chain holds a batch's frames");

extern "C" size_t trt_ansi_delta_capacity(int width, int rows)
{
    if (!trt_delta_size_ok(width, rows))
        return 0;
    return (size_t)std::max(trt_ansi_text_bytes(width, rows), trt_delta_bound(width, rows));
}

extern "C" size_t trt_ansi_delta_half_capacity(int width, int rows)
{
    if (!trt_delta_half_size_ok(width, rows))
        return 0;
    return (size_t)std::max(trt_ansi_half_text_bytes(width, rows), trt_delta_half_bound(width, rows));
}

extern "C" size_t trt_ansi256_delta_capacity(int width, int rows)
{
    return (size_t)trt_delta256_capacity(width, rows);
}

extern "C" size_t trt_ansi256_delta_half_capacity(int width, int rows)
{
    return (size_t)trt_delta256_half_capacity(width, rows);
}

// What a kind of MEASURED text -- one whose length depends on the picture, so that the device reports it: the four delta texts and the sixel
// image (below) -- says of a frame size: whether it has such a text, the refusal where it has none, and the room any text of the size fits.
struct MeasuredText
{
    int (*size_ok)(int width, long long rows);
    const char *no_text; // with the width, the rows and the two limits
    int max_width, max_rows;
    size_t (*capacity)(int width, int rows);
};
static const MeasuredText kDeltaText[kDeltaKinds] = { // by DeltaKind
    {trt_delta_size_ok, "%d x %d: a delta text has 1 to %d cells per row and 1 to %d rows", TRT_DELTA_MAX_WIDTH, TRT_DELTA_MAX_ROWS, trt_ansi_delta_capacity},
    {trt_delta_half_size_ok, "%d x %d: a half-block delta text has 1 to %d cells per row and 1 to %d text rows", TRT_DELTA_HALF_MAX_WIDTH, TRT_DELTA_HALF_MAX_TEXT_ROWS,
     trt_ansi_delta_half_capacity},
    {trt_delta256_size_ok, "%d x %d: a 256-colour delta text has 1 to %d cells per row and 1 to %d rows", TRT_DELTA256_MAX_WIDTH, TRT_DELTA256_MAX_ROWS,
     trt_ansi256_delta_capacity},
    {trt_delta256_half_size_ok, "%d x %d: a half-block 256-colour delta text has 1 to %d cells per row and 1 to %d text rows", TRT_DELTA256_HALF_MAX_WIDTH,
     TRT_DELTA256_HALF_MAX_TEXT_ROWS, trt_ansi256_delta_half_capacity}};
// the shape of a kind's cells: its tiles are of the text rows' cells
static bool delta_half_cells(DeltaKind kind) { return kind == kDeltaHalf || kind == kDelta256Half; }
static const MeasuredText kSixelText = {trt_sixel_size_ok, "%d x %d: a sixel image has 1 to %d pixels a row and 1 to %d rows", TRT_SIXEL_MAX, TRT_SIXEL_MAX,
                                        trt_sixel_capacity};

// the frames a text of the kind exists for: TRT_OK, or the refusal
static int check_measured_size(const MeasuredText &k, int width, int rows)
{
    return k.size_ok(width, rows) ? TRT_OK : fail(TRT_ERR_ARGUMENT, k.no_text, width, rows, k.max_width, k.max_rows);
}

// What the render entries of a measured text refuse before anything is enqueued: what trt_render_device_batch_rgb8 refuses for the n cameras,
// a size without a text, and a `text` -- the caller's buffer, on the device or on the host -- without room for n texts of the size, which
// `no_room(need)` words.
template <class NoRoom>
static int check_render_measured(const trt_context *ctx, const MeasuredText &k, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                 const void *text, size_t capacity_bytes, const void *bytes, NoRoom no_room)
{
    if (!bytes)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    int rc = rowset_valid(rows) ? check_measured_size(k, rows->width, trt_rowset_rows(rows)) : TRT_OK;
    if (rc)
        return rc;
    // the rest as the RGB8 entry checks it, whose frame these sizes let fit
    rc = check_render_arguments(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, text, (size_t)-1, kBytes);
    if (rc)
        return rc;
    const size_t need = (size_t)n * k.capacity(rows->width, trt_rowset_rows(rows));
    if (capacity_bytes < need)
        return no_room(need);
    return check_batch_tables(ctx, n);
}

// The copy-out of a measured text's host entries: the n lengths at d_delta_bytes read back and held against `room`, the bytes at d_text
// (`too_long()` words the refusal), then exactly their sum through pinned staging of `staged(sum)` bytes into `text` -- two transfers
// whatever n is -- and the lengths into `bytes`.  *sum: what was copied.
template <class Staged, class TooLong>
static int copy_out_measured(trt_context *ctx, int n, size_t room, char *text, size_t *bytes, unsigned long long *sum, Staged staged, TooLong too_long)
{
    unsigned long long length[TRT_BATCH_MAX] = {};
    HIP_TRY(hipMemcpyAsync(ctx->h_staging.ptr, ctx->d_delta_bytes.ptr, sizeof length[0] * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(length, ctx->h_staging.ptr, sizeof length[0] * n);
    *sum = 0;
    for (int b = 0; b < n; b++)
    {
        if (length[b] > room - *sum)
            return too_long();
        *sum += length[b];
    }
    if (*sum)
    {
        HIP_TRY(ctx->h_staging.reserve(staged((size_t)*sum)));
        HIP_TRY(hipMemcpyAsync(ctx->h_staging.ptr, ctx->d_text.ptr, (size_t)*sum, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        memcpy(text, ctx->h_staging.ptr, (size_t)*sum);
    }
    for (int b = 0; b < n; b++)
        bytes[b] = (size_t)length[b];
    return TRT_OK;
}

// measure, offsets, write on `stream` for the pairs (d_shown, frame 0), (frame 0, frame 1) ... of the n frames at d_frames, of the full text's
// cells or of half-block cells (the tiles are then of the text rows' cells), in 24-bit colour or in the palette: text b at d_text + base + the lengths before it, its length at
// d_bytes[b]; capacity_bytes: the bytes at d_text; marks: four events, recorded around and between the launches (the ..._kernel_times entries)
static int launch_ansi_delta(trt_context *ctx, hipStream_t stream, DeltaKind kind, const unsigned char *d_shown, const unsigned char *d_frames, int n, int width, int rows,
                             void *d_text, size_t capacity_bytes, unsigned long long base, unsigned long long *d_bytes, const Event *marks = nullptr)
{
    static const struct
    {
        void (*measure)(const unsigned char *, const unsigned char *, int, int, unsigned *);
        void (*write)(const unsigned char *, const unsigned char *, int, int, const unsigned long long *, unsigned char *, unsigned long long);
    } kernels[kDeltaKinds] = {{trt::ansi_delta_chain_measure_kernel, trt::ansi_delta_chain_write_kernel},
                              {trt::ansi_delta_half_chain_measure_kernel, trt::ansi_delta_half_chain_write_kernel},
                              {trt::ansi256_delta_chain_measure_kernel, trt::ansi256_delta_chain_write_kernel},
                              {trt::ansi256_delta_half_chain_measure_kernel, trt::ansi256_delta_half_chain_write_kernel}};
    const unsigned long long cells = (unsigned long long)width * (unsigned long long)(delta_half_cells(kind) ? trt_ansi_half_text_rows(rows) : rows),
                             tiles = trt_delta_tiles(cells);
    const size_t all = (size_t)tiles * (size_t)n;
    if (ctx->d_delta_tile_bytes.capacity < all || ctx->d_delta_tile_at.capacity < all)
        HIP_TRY(hipStreamSynchronize(stream)); // a text in flight may still use the old sums
    HIP_TRY(ctx->d_delta_tile_bytes.reserve(all));
    HIP_TRY(ctx->d_delta_tile_at.reserve(all));
    const dim3 grid((unsigned)tiles, (unsigned)n);
    if (marks)
        HIP_TRY(hipEventRecord(marks[0], stream));
    hipLaunchKernelGGL(kernels[kind].measure, grid, dim3(TRT_DELTA_BLOCK), 0, stream, d_shown, d_frames, width, rows, ctx->d_delta_tile_bytes.ptr);
    if (marks)
        HIP_TRY(hipEventRecord(marks[1], stream));
    hipLaunchKernelGGL(trt::ansi_delta_chain_offsets_kernel, dim3(1), dim3(TRT_DELTA_SCAN_BLOCK), 0, stream, (const unsigned *)ctx->d_delta_tile_bytes.ptr, tiles, (unsigned)n,
                       base, ctx->d_delta_tile_at.ptr, d_bytes);
    if (marks)
        HIP_TRY(hipEventRecord(marks[2], stream));
    hipLaunchKernelGGL(kernels[kind].write, grid, dim3(TRT_DELTA_BLOCK), 0, stream, d_shown, d_frames, width, rows, (const unsigned long long *)ctx->d_delta_tile_at.ptr,
                       (unsigned char *)d_text, (unsigned long long)capacity_bytes);
    if (marks)
        HIP_TRY(hipEventRecord(marks[3], stream));
    HIP_TRY(hipGetLastError());
    return TRT_OK;
}

// The formatting alone, all sixteen entries: trt_ansi[256]_delta(_half)_from_rgb8_device with d_next as a chain of one frame,
// trt_ansi[256]_delta(_half)_chain_from_rgb8_device, and with `ms` their ..._kernel_times forms, which are synchronous
static int delta_from_rgb8(trt_context *ctx, DeltaKind kind, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text, size_t capacity_bytes,
                           unsigned long long *d_bytes, float *ms = nullptr)
{
    if (!ctx || !d_shown_rgb8 || !d_frames_rgb8 || !d_text || !d_bytes)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (n < 1 || n > TRT_BATCH_MAX)
        return fail(TRT_ERR_ARGUMENT, "a chain has 1 to %d frames, %d given", TRT_BATCH_MAX, n);
    int rc = check_measured_size(kDeltaText[kind], width, rows);
    if (rc)
        return rc;
    const size_t need = (size_t)n * kDeltaText[kind].capacity(width, rows);
    if (capacity_bytes < need)
        return fail(TRT_ERR_CAPACITY, "%d delta text(s) of %d x %d need room for %zu B, %zu given", n, width, rows, need, capacity_bytes);
    HIP_TRY(hipSetDevice(ctx->device));
    Event marks[4];
    if (ms)
        for (Event &e : marks)
            HIP_TRY(e.create());
    rc = launch_ansi_delta(ctx, ctx->stream, kind, (const unsigned char *)d_shown_rgb8, (const unsigned char *)d_frames_rgb8, n, width, rows, d_text, capacity_bytes, 0, d_bytes,
                           ms ? marks : nullptr);
    if (!ms)
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (rc)
        return rc;
    for (int k = 0; k < 3; k++)
        HIP_TRY(hipEventElapsedTime(&ms[k], marks[k], marks[k + 1]));
    return TRT_OK;
}

extern "C" int trt_ansi_delta_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                               size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDeltaFull, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi_delta_half_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                                    size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDeltaHalf, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi_delta_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                           size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDeltaFull, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi_delta_half_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                                size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDeltaHalf, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi_delta_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                     size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDeltaFull, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi_delta_half_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                          size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDeltaHalf, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi_delta_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                 size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDeltaFull, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi_delta_half_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                      size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDeltaHalf, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi256_delta_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                                size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDelta256, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi256_delta_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                            size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDelta256, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi256_delta_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                      size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDelta256, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi256_delta_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                  size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDelta256, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi256_delta_half_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                                     size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDelta256Half, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi256_delta_half_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                                 size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDelta256Half, d_shown_rgb8, d_next_rgb8, 1, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

extern "C" int trt_ansi256_delta_half_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                           size_t capacity_bytes, unsigned long long *d_bytes)
{
    return delta_from_rgb8(ctx, kDelta256Half, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes);
}

extern "C" int trt_ansi256_delta_half_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows, void *d_text,
                                                       size_t capacity_bytes, unsigned long long *d_bytes, float *ms)
{
    return ms ? delta_from_rgb8(ctx, kDelta256Half, d_shown_rgb8, d_frames_rgb8, n, width, rows, d_text, capacity_bytes, d_bytes, ms) : fail(TRT_ERR_ARGUMENT, "NULL argument");
}

// ---- the render entries of the four delta texts: one shown frame, which remembers the kind of text it was sent as ----

extern "C" int trt_ansi_delta_reset(trt_context *ctx)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    ctx->shown_valid = false;
    return TRT_OK;
}

// check_render_measured for n delta texts of the kind
static int check_render_delta(const trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, const void *text,
                              size_t capacity_bytes, const void *bytes, DeltaKind kind)
{
    return check_render_measured(ctx, kDeltaText[kind], cameras, n, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, [&](size_t need) {
        return fail(TRT_ERR_CAPACITY, "%d text(s) of %d x %d owned rows need room for %zu B, %zu given", n, rows->width, trt_rowset_rows(rows), need, capacity_bytes);
    });
}

static bool same_rowset(const trt_rowset &a, const trt_rowset &b)
{
    return a.width == b.width && a.height == b.height && a.tile_rows == b.tile_rows && a.tile_first == b.tile_first && a.tile_step == b.tile_step;
}

// trt_render_device_ansi_delta and trt_render_device_batch_ansi_delta, their _half forms and the ansi256 forms of the four: n cameras as n texts back to back, text 0
// against the shown frame.  `batch` as in render_host_as: the batch route, which picks the render kernel's BATCH form and counts for
// trt_batch_info; otherwise n is 1 and the frame is the single frame's launch.
static int render_device_delta(trt_context *ctx, const Camera *cameras, int n, bool batch, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                               size_t capacity_bytes, unsigned long long *d_bytes, DeltaKind kind)
{
    int rc = check_render_delta(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kind);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int width = rows->width, owned = trt_rowset_rows(rows);
    const size_t frame = (size_t)owned * width * 3;
    const bool keyframe = !(ctx->shown_valid && ctx->shown_kind == kind && same_rowset(ctx->shown_rows, *rows));
    const int into = ctx->shown_at ^ 1;
    if (ctx->d_delta_frames[into].capacity < frame * n)
    { // only the buffer rendered into grows, with nothing in flight that uses it: a buffer that grows loses its contents, and the other one holds the shown frame
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx->d_delta_frames[into].reserve(frame * n));
    }
    unsigned char *const frames = ctx->d_delta_frames[into].ptr;
    ctx->shown_valid = false; // a call that fails from here on has forgotten the shown frame
    // the new frames' bytes, back to back: the RGB8 form of the ordered mean (the reference-order kernel: its doubles through quantize_kernel); a
    // batch in one launch, split for LDS or one launch per camera, as trt_render_device_batch_rgb8 decides
    rc = batch ? render_device_batch(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, frames, frame * n, kBytes)
               : render_device_on(ctx, cameras, rows, bounce_limit, rays_per_pixel, frames, frame, 0, kEntryWhole, kBytes);
    if (rc)
        return rc;
    if (keyframe)
    { // text 0 is the whole text of frame 0, as trt_render_device_ansi[256][_half] writes it; the chain of the pairs behind it starts where that text ends
        static const Output kWhole[kDeltaKinds] = {kText, kHalfText, kText256, kHalfText256};
        const unsigned long long whole = frame_bytes(kWhole[kind], width, owned);
        launch_text_from_rgb8(ctx->stream, kWhole[kind], frames, width, owned, d_text);
        hipLaunchKernelGGL(trt::ansi_delta_keyframe_bytes_kernel, dim3(1), dim3(1), 0, ctx->stream, d_bytes, whole);
        HIP_TRY(hipGetLastError());
        if (n > 1)
            rc = launch_ansi_delta(ctx, ctx->stream, kind, frames, frames + frame, n - 1, width, owned, d_text, capacity_bytes, whole, d_bytes + 1);
    }
    else // a shown frame of this size: the other buffer holds it, untouched since the call that rendered it
        rc = launch_ansi_delta(ctx, ctx->stream, kind, ctx->d_delta_frames[ctx->shown_at].ptr + (size_t)ctx->shown_frame * frame, frames, n, width, owned, d_text, capacity_bytes,
                               0, d_bytes);
    if (rc)
        return rc;
    ctx->shown_at = into; // the buffers flip: the last frame is the shown one from here on, where it was rendered
    ctx->shown_frame = n - 1;
    ctx->shown_rows = *rows;
    ctx->shown_kind = kind;
    ctx->shown_valid = true;
    return TRT_OK;
}

extern "C" int trt_render_device_ansi_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                            size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDeltaFull);
}

extern "C" int trt_render_device_ansi_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                                 size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDeltaHalf);
}

extern "C" int trt_render_device_batch_ansi_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                                  size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDeltaFull);
}

extern "C" int trt_render_device_batch_ansi_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                                       void *d_text, size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDeltaHalf);
}

extern "C" int trt_render_device_ansi256_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                              size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDelta256);
}

extern "C" int trt_render_device_batch_ansi256_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                                    size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDelta256);
}

extern "C" int trt_render_device_ansi256_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                                   size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDelta256Half);
}

extern "C" int trt_render_device_batch_ansi256_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                                         size_t capacity_bytes, unsigned long long *d_bytes)
{
    return render_device_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes, kDelta256Half);
}

// The copy-out of the eight host entries, timed as `name` under print_host_times(): the n texts in the context's text buffer, their
// lengths read back, then exactly their sum -- two transfers whatever n is.
static int render_host_delta(trt_context *ctx, const Camera *cameras, int n, bool batch, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                             size_t capacity_bytes, size_t *bytes, DeltaKind kind, const char *name)
{
    int rc = check_render_delta(ctx, cameras, n, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kind);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t room = (size_t)n * kDeltaText[kind].capacity(rows->width, trt_rowset_rows(rows));
    if (ctx->d_text.capacity < room || ctx->d_delta_bytes.capacity < (size_t)n)
        HIP_TRY(hipStreamSynchronize(ctx->stream)); // a text in flight may still be written to the old buffers
    HIP_TRY(ctx->d_text.reserve(room));
    HIP_TRY(ctx->d_delta_bytes.reserve((size_t)n));
    // Pinned staging.  A single frame: its text's capacity, once, so that a moving picture does not allocate pinned memory again and again as
    // its texts grow.  A batch: the lengths now and the texts' sum when it is known -- n capacities are hundreds of MB at 1920x1080.
    HIP_TRY(ctx->h_staging.reserve(batch ? sizeof(unsigned long long) * TRT_BATCH_MAX : room));
    const double t_begin = host_now_ms();
    rc = render_device_delta(ctx, cameras, n, batch, rows, bounce_limit, rays_per_pixel, ctx->d_text.ptr, room, ctx->d_delta_bytes.ptr, kind);
    if (rc)
        return rc;
    unsigned long long sum = 0;
    rc = copy_out_measured(ctx, n, room, text, bytes, &sum, [](size_t copied) { return copied; },
                           [&] { return fail(TRT_ERR_CAPACITY, "%d text(s) of more than %zu B", n, room); });
    if (rc)
    { // the host did not get the texts: the terminal does not show these frames
        ctx->shown_valid = false;
        return rc;
    }
    if (print_host_times())
        fprintf(stderr, "%s: %.3f ms for %d text(s) of %llu bytes\n", name, host_now_ms() - t_begin, n, sum);
    return TRT_OK;
}

extern "C" int trt_render_host_ansi_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                          size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDeltaFull, "trt_render_host_ansi_delta");
}

extern "C" int trt_render_host_ansi_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                               size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDeltaHalf, "trt_render_host_ansi_delta_half");
}

extern "C" int trt_render_host_batch_ansi_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                                size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDeltaFull, "trt_render_host_batch_ansi_delta");
}

extern "C" int trt_render_host_batch_ansi_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                                     size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDeltaHalf, "trt_render_host_batch_ansi_delta_half");
}

extern "C" int trt_render_host_ansi256_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                            size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDelta256, "trt_render_host_ansi256_delta");
}

extern "C" int trt_render_host_batch_ansi256_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                                  size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDelta256, "trt_render_host_batch_ansi256_delta");
}

extern "C" int trt_render_host_ansi256_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                                 size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, camera, 1, false, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDelta256Half, "trt_render_host_ansi256_delta_half");
}

extern "C" int trt_render_host_batch_ansi256_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                                       size_t capacity_bytes, size_t *bytes)
{
    return render_host_delta(ctx, cameras, n, true, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, kDelta256Half, "trt_render_host_batch_ansi256_delta_half");
}

// ---- the sixel image (trt_sixel.h: the format, its position map and its lane map; trt_sixel.hpp: the kernels).  Its length depends on the
// picture, so it goes the delta texts' way: the frame's RGB8 bytes, then measure, offsets, write ----

extern "C" size_t trt_sixel_capacity(int width, int rows)
{
    return (size_t)trt_sixel_capacity_bytes(width, rows);
}

// measure, offsets, write on `stream` for the frame of width x rows at d_rgb8: the text at d_text, any alignment, its length at *d_bytes
static int launch_sixel(trt_context *ctx, hipStream_t stream, const unsigned char *d_rgb8, int width, int rows, void *d_text, unsigned long long *d_bytes)
{
    const size_t bands = (size_t)trt_sixel_bands(rows);
    if (ctx->d_sixel_masks.capacity < bands * TRT_SIXEL_MASK_WORDS || ctx->d_sixel_counts.capacity < bands || ctx->d_sixel_band_at.capacity < bands)
        HIP_TRY(hipStreamSynchronize(stream)); // an image in flight may still use the old masks
    HIP_TRY(ctx->d_sixel_masks.reserve(bands * TRT_SIXEL_MASK_WORDS));
    HIP_TRY(ctx->d_sixel_counts.reserve(bands));
    HIP_TRY(ctx->d_sixel_band_at.reserve(bands));
    const trt_text_split split = trt_sixel_row_split((unsigned long long)d_text, width);
    const unsigned tiles = (trt_sixel_slots(&split) + TRT_SIXEL_BLOCK - 1) / TRT_SIXEL_BLOCK;
    hipLaunchKernelGGL(trt::sixel_measure_kernel, dim3((unsigned)bands), dim3(TRT_SIXEL_BLOCK), 0, stream, d_rgb8, width, rows, ctx->d_sixel_masks.ptr, ctx->d_sixel_counts.ptr);
    hipLaunchKernelGGL(trt::sixel_offsets_kernel, dim3(1), dim3(TRT_SIXEL_SCAN_BLOCK), 0, stream, (const unsigned *)ctx->d_sixel_counts.ptr, width, rows,
                       ctx->d_sixel_band_at.ptr, (unsigned char *)d_text, d_bytes);
    hipLaunchKernelGGL(trt::sixel_write_kernel, dim3(tiles, (unsigned)bands), dim3(TRT_SIXEL_BLOCK), 0, stream, d_rgb8, width, rows, (const unsigned *)ctx->d_sixel_masks.ptr,
                       (const unsigned long long *)ctx->d_sixel_band_at.ptr, (unsigned char *)d_text);
    HIP_TRY(hipGetLastError());
    return TRT_OK;
}

extern "C" int trt_sixel_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes)
{
    if (!ctx || !d_rgb8 || !d_text || !d_bytes)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    const int rc = check_measured_size(kSixelText, width, rows);
    if (rc)
        return rc;
    const size_t need = trt_sixel_capacity(width, rows);
    if (capacity_bytes < need)
        return fail(TRT_ERR_CAPACITY, "a sixel image of %d x %d needs room for %zu B, %zu given", width, rows, need, capacity_bytes);
    HIP_TRY(hipSetDevice(ctx->device));
    return launch_sixel(ctx, ctx->stream, (const unsigned char *)d_rgb8, width, rows, d_text, d_bytes);
}

// check_render_measured for the one image
static int check_sixel_render(const trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, const void *text,
                              size_t capacity_bytes, const void *bytes)
{
    return check_render_measured(ctx, kSixelText, camera, 1, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, [&](size_t need) {
        return fail(TRT_ERR_CAPACITY, "a sixel image of %d x %d owned rows needs room for %zu B, %zu given", rows->width, trt_rowset_rows(rows), need, capacity_bytes);
    });
}

extern "C" int trt_render_device_sixel(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, void *d_text,
                                       size_t capacity_bytes, unsigned long long *d_bytes)
{
    int rc = check_sixel_render(ctx, camera, rows, bounce_limit, rays_per_pixel, d_text, capacity_bytes, d_bytes);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const int width = rows->width, owned = trt_rowset_rows(rows);
    const size_t frame = (size_t)owned * width * 3;
    if (ctx->d_sixel_frame.capacity < frame)
    {
        HIP_TRY(hipStreamSynchronize(ctx->stream)); // an image in flight may still be formatted from the old bytes
        HIP_TRY(ctx->d_sixel_frame.reserve(frame));
    }
    // the frame's bytes: the RGB8 form of the ordered mean (the reference-order kernel: its doubles through quantize_kernel)
    rc = render_device_on(ctx, camera, rows, bounce_limit, rays_per_pixel, ctx->d_sixel_frame.ptr, frame, 0, kEntryWhole, kBytes);
    if (rc)
        return rc;
    return launch_sixel(ctx, ctx->stream, ctx->d_sixel_frame.ptr, width, owned, d_text, d_bytes);
}

// the image in the context's text buffer, its length read back, then exactly that many bytes through the pinned staging
extern "C" int trt_render_host_sixel(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel, char *text,
                                     size_t capacity_bytes, size_t *bytes)
{
    int rc = check_sixel_render(ctx, camera, rows, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t room = trt_sixel_capacity(rows->width, trt_rowset_rows(rows));
    if (ctx->d_text.capacity < room || ctx->d_delta_bytes.capacity < 1)
        HIP_TRY(hipStreamSynchronize(ctx->stream)); // a text in flight may still be written to the old buffers
    HIP_TRY(ctx->d_text.reserve(room));
    HIP_TRY(ctx->d_delta_bytes.reserve(1));
    HIP_TRY(ctx->h_staging.reserve(sizeof(unsigned long long)));
    const double t_begin = host_now_ms();
    rc = trt_render_device_sixel(ctx, camera, rows, bounce_limit, rays_per_pixel, ctx->d_text.ptr, room, ctx->d_delta_bytes.ptr);
    if (rc)
        return rc;
    // Pinned staging grows with the images' lengths, not to the capacity -- 240 colours in every band are 83 MB at 1920x1080 and rare -- and
    // in steps of a power of two, so that a moving picture whose images grow does not allocate pinned memory frame after frame
    const auto staged = [&](size_t length) {
        size_t bytes = 4096;
        while (bytes < length)
            bytes *= 2;
        return std::min(bytes, std::max(room, sizeof(unsigned long long)));
    };
    unsigned long long length = 0;
    rc = copy_out_measured(ctx, 1, room, text, bytes, &length, staged, [&] { return fail(TRT_ERR_CAPACITY, "an image of more than %zu B", room); });
    if (rc)
        return rc;
    if (print_host_times())
        fprintf(stderr, "trt_render_host_sixel: %.3f ms for an image of %llu bytes\n", host_now_ms() - t_begin, length);
    return TRT_OK;
}
