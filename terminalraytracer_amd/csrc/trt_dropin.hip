// trt_dropin.hip -- section 1 of include/trt_hip.h: project_scene (TRT.c:966) / render_frame and the default context behind them.
// Compiled for gfx950 only, with -ffp-contract=off (see trt_device.hpp).
#include "trt_context.hpp"

using namespace trt_impl;

namespace
{
trt_context *g_default = nullptr;
int g_default_device = 0;
// The reference's project_scene is a pure function of its arguments and may be called from several threads; the drop-in
// shares one device context, so calls on the default context take turns.
std::mutex g_default_mutex;

int g_default_specular = -1; // trt_set_default_specular: 0 / 1 for the default context until trt_shutdown; -1: what a new context starts with
int g_default_sky_filter = -1; // trt_set_default_sky_filter: the same for the sky filter

int default_context(trt_context **out)
{
    if (!g_default)
    {
        int rc = trt_create(g_default_device, &g_default);
        if (rc)
            return rc;
        if (g_default_specular >= 0)
            g_default->specular = g_default_specular;
        if (g_default_sky_filter >= 0)
            g_default->sky_filter = g_default_sky_filter;
    }
    *out = g_default;
    return TRT_OK;
}
} // namespace

extern "C" int trt_init(int device)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    if (g_default && g_default->device != device)
    {
        trt_destroy(g_default);
        g_default = nullptr;
    }
    g_default_device = device;
    trt_context *ctx;
    return default_context(&ctx);
}

extern "C" int trt_shutdown(void)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    int rc = trt_destroy(g_default);
    g_default = nullptr;
    g_default_specular = -1;
    g_default_sky_filter = -1;
    return rc;
}

extern "C" int trt_upload_skybox(const Skybox *skybox)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    if (!skybox)
        return fail(TRT_ERR_ARGUMENT, "skybox is NULL");
    trt_context *ctx;
    int rc = default_context(&ctx);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return upload_skybox(ctx, skybox);
}

extern "C" int trt_invalidate_skybox(void)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    if (g_default)
        g_default->sky_dim = -1;
    return TRT_OK;
}

// The caller owns the scene and may have edited it since the last frame (main() rewrites the camera every frame,
// TRT.c:1327-1336): primitives are a few KB and are re-sent; the 6*dim*dim texels only when the face pointers, the dimension
// or the texel stamp changed.  With g_default_mutex held.
static int refresh_default_scene(trt_context *ctx, const Scene *scene)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const double t_begin = host_now_ms();
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->have_scene = false;
    int rc = upload_primitives(ctx, scene, true);
    if (rc)
        return rc;
    bool same_sky = ctx->sky_dim == scene->skybox.dim;
    for (int f = 0; f < 6 && same_sky; f++)
        same_sky = scene->skybox.colors[f] && ctx->sky_faces[f] == scene->skybox.colors[f];
    same_sky = same_sky && scene->skybox.dim > 0 && ctx->sky_stamp == skybox_stamp(&scene->skybox);
    if (!same_sky)
    {
        rc = upload_skybox(ctx, &scene->skybox);
        if (rc)
            return rc;
    }
    ctx->have_scene = true;
    if (print_host_times())
        fprintf(stderr, "trt_render_frame: scene upload %.3f ms\n", host_now_ms() - t_begin);
    return TRT_OK;
}

// The drop-in entries (project_scene, trt_render_frame, trt_render_frame_rgb8, trt_render_frame_ansi, trt_render_frame_ansi_half, trt_render_frame_kitty, trt_render_frame_ansi256, trt_render_frame_ansi256_half) take the scene with every call.  A scene whose
// primitives differ from the previous call's on `moving_after` consecutive calls is treated as MOVING: its candidate tables are
// rebuilt per call the cheap way (one family per sphere, no patches); after `still_after` consecutive unchanged calls the full
// tables are built once.  moving_after = 0: never (every change builds the full tables).  Defaults 2 and 3.  Frames are
// bit-identical either way.  trt_scene_is_moving() says whether the default context currently treats its scene as moving.
extern "C" int trt_set_scene_policy(int moving_after, int still_after)
{
    if (moving_after < 0 || still_after < 1)
        return fail(TRT_ERR_ARGUMENT, "scene policy %d, %d", moving_after, still_after);
    std::lock_guard<std::mutex> turn(g_default_mutex);
    g_moving_after = moving_after;
    g_still_after = still_after;
    // "never": upload_primitives only ever sets the flag from a run of changes and clears it after still_after unchanged calls, so a
    // context that is moving now would go on building the cheap tables for every further change.  Cleared here, the next call finds
    // tables built for a moving scene under a scene that is not, and builds the full ones.
    if (moving_after == 0 && g_default)
        g_default->moving_scene = false;
    return TRT_OK;
}

// The specular extension (trt_set_specular) for the default context, which the callers of the drop-in entries cannot reach: it holds
// for the context that exists and for one that a later call creates, until trt_shutdown.
extern "C" int trt_set_default_specular(int on)
{
    if (on != 0 && on != 1)
        return fail(TRT_ERR_ARGUMENT, "specular %d (0 or 1)", on);
    std::lock_guard<std::mutex> turn(g_default_mutex);
    g_default_specular = on;
    if (g_default)
        g_default->specular = on;
    return TRT_OK;
}

// ... and the sky filter (trt_set_sky_filter), in the same way.
extern "C" int trt_set_default_sky_filter(int mode)
{
    if (mode != TRT_SKY_NEAREST && mode != TRT_SKY_BILINEAR)
        return fail(TRT_ERR_ARGUMENT, "sky filter %d (TRT_SKY_NEAREST or TRT_SKY_BILINEAR)", mode);
    std::lock_guard<std::mutex> turn(g_default_mutex);
    g_default_sky_filter = mode;
    if (g_default)
        g_default->sky_filter = mode;
    return TRT_OK;
}

extern "C" int trt_scene_is_moving(void)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    return g_default && g_default->moving_scene ? 1 : 0;
}

// trt_hip_diag.h: the tests' handle on the default context and what it has built so far
extern "C" trt_context *trt_default_context(void)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    return g_default;
}

extern "C" int trt_build_counts(trt_context *ctx, unsigned long long *table_builds, unsigned long long *skybox_uploads)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    if (table_builds)
        *table_builds = ctx->table_builds;
    if (skybox_uploads)
        *skybox_uploads = ctx->skybox_uploads;
    return TRT_OK;
}

// What the drop-in entries do once their own arguments have passed: the default context's turn, the caller's scene on it, and
// render(ctx, rows) over the whole screen.
template <class Render>
static int render_default_frame(const Scene *scene, int width, int height, Render render)
{
    std::lock_guard<std::mutex> turn(g_default_mutex);
    trt_context *ctx;
    int rc = default_context(&ctx);
    if (rc)
        return rc;
    rc = refresh_default_scene(ctx, scene);
    if (rc)
        return rc;
    const trt_rowset whole = {width, height, height, 0, 1};
    return render(ctx, &whole);
}

extern "C" int trt_render_frame(const Scene *scene, Screen *screen, int bounce_limit, int rays_per_pixel)
{
    if (!scene || !screen || !screen->pixels)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (screen->width <= 0 || screen->height <= 0)
        return fail(TRT_ERR_ARGUMENT, "screen %d x %d", screen->width, screen->height);
    return render_default_frame(scene, screen->width, screen->height, [&](trt_context *ctx, const trt_rowset *whole) {
        return trt_render_host(ctx, &scene->camera, whole, bounce_limit, rays_per_pixel, screen->pixels);
    });
}

// north_star's name for the entry: the frame producer with the two macros of TRT.c:54, :58 as run-time values
extern "C" int render_frame(const Scene *scene, Screen *screen, int bounce_limit, int rays_per_pixel)
{
    return trt_render_frame(scene, screen, bounce_limit, rays_per_pixel);
}

// every kind whose length the size fixes -- the bytes, the four character-cell texts, the kitty image: `render` is the kind's host entry,
// `has_size`: whether the kind exists at this size
template <class T>
static int render_frame_as(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, T *out,
                           int (*render)(trt_context *, const Camera *, const trt_rowset *, int, int, T *), bool has_size = true)
{
    if (!scene || !out)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (width <= 0 || height <= 0 || !has_size)
        return fail(TRT_ERR_ARGUMENT, "screen %d x %d", width, height);
    return render_default_frame(scene, width, height, [&](trt_context *ctx, const trt_rowset *whole) {
        return render(ctx, &scene->camera, whole, bounce_limit, rays_per_pixel, out);
    });
}

extern "C" int trt_render_frame_rgb8(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, unsigned char *rgb)
{
    return render_frame_as(scene, width, height, bounce_limit, rays_per_pixel, rgb, trt_render_host_rgb8);
}

extern "C" int trt_render_frame_ansi(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_frame_as(scene, width, height, bounce_limit, rays_per_pixel, text, trt_render_host_ansi);
}

extern "C" int trt_render_frame_ansi_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_frame_as(scene, width, height, bounce_limit, rays_per_pixel, text, trt_render_host_ansi_half);
}

extern "C" int trt_render_frame_kitty(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_frame_as(scene, width, height, bounce_limit, rays_per_pixel, text, trt_render_host_kitty, trt_kitty_bytes(width, height) != 0);
}

extern "C" int trt_render_frame_ansi256(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_frame_as(scene, width, height, bounce_limit, rays_per_pixel, text, trt_render_host_ansi256);
}

extern "C" int trt_render_frame_ansi256_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text)
{
    return render_frame_as(scene, width, height, bounce_limit, rays_per_pixel, text, trt_render_host_ansi256_half);
}

// the shown frame is the default context's: trt_shutdown forgets it with the context.  `capacity` and `render`: those of the kind
static int render_frame_delta(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text, size_t capacity_bytes, size_t *bytes,
                              size_t (*capacity)(int, int),
                              int (*render)(trt_context *, const Camera *, const trt_rowset *, int, int, char *, size_t, size_t *))
{
    if (!scene || !text || !bytes)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (width <= 0 || height <= 0 || capacity(width, height) == 0)
        return fail(TRT_ERR_ARGUMENT, "screen %d x %d", width, height);
    if (capacity_bytes < capacity(width, height))
        return fail(TRT_ERR_CAPACITY, "the text of %d x %d needs room for %zu B, %zu given", width, height, capacity(width, height), capacity_bytes);
    return render_default_frame(scene, width, height, [&](trt_context *ctx, const trt_rowset *whole) {
        return render(ctx, &scene->camera, whole, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes);
    });
}

extern "C" int trt_render_frame_ansi_delta(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text, size_t capacity_bytes,
                                           size_t *bytes)
{
    return render_frame_delta(scene, width, height, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, trt_ansi_delta_capacity, trt_render_host_ansi_delta);
}

extern "C" int trt_render_frame_ansi_delta_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text, size_t capacity_bytes,
                                                size_t *bytes)
{
    return render_frame_delta(scene, width, height, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, trt_ansi_delta_half_capacity,
                              trt_render_host_ansi_delta_half);
}

extern "C" int trt_render_frame_ansi256_delta(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text, size_t capacity_bytes,
                                              size_t *bytes)
{
    return render_frame_delta(scene, width, height, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, trt_ansi256_delta_capacity,
                              trt_render_host_ansi256_delta);
}

extern "C" int trt_render_frame_ansi256_delta_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text, size_t capacity_bytes,
                                                   size_t *bytes)
{
    return render_frame_delta(scene, width, height, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, trt_ansi256_delta_half_capacity,
                              trt_render_host_ansi256_delta_half);
}

// the sixel image: a text whose length the call reports, as the delta texts', but of the frame alone -- no shown frame is read or changed
extern "C" int trt_render_frame_sixel(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text, size_t capacity_bytes, size_t *bytes)
{
    return render_frame_delta(scene, width, height, bounce_limit, rays_per_pixel, text, capacity_bytes, bytes, trt_sixel_capacity, trt_render_host_sixel);
}

extern "C" void project_scene(Scene *scene, Screen *screen)
{
    const int rc = trt_render_frame(scene, screen, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL);
    if (rc != TRT_OK)
    {
        fprintf(stderr, "project_scene (libtrt_hip): %s\n", trt_last_error());
        abort();
    }
}

