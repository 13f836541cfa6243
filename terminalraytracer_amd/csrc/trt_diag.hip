// trt_diag.hip -- include/trt_hip_diag.h: loop diagnostics, table read-backs, device self-tests, single-ray probes, test hooks.
// Nothing here is needed to produce a frame.
// Compiled for gfx950 only, with -ffp-contract=off (see trt_device.hpp).
#define TRT_UNIT_DIAG 1 // this unit is the home of the kernels that are not templates (trt_common.hpp, trt_simple.hpp)
#include "trt_context.hpp"
#include "trt_simple.hpp"

using namespace trt_impl;

namespace trt_impl
{
void allow_large_lds_diag(const trt_context *ctx)
{
    (void)hipFuncSetAttribute((const void *)trt::probe_rays_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rays_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rounds_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rounds_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rounds_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rounds_kernel<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rays_kernel<false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rounds_kernel<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::probe_rounds_kernel<true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
}
} // namespace trt_impl

extern "C" int trt_set_list_pool_words(trt_context *ctx, size_t words)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    const int rc = refuse_if_shared(ctx, "trt_set_list_pool_words");
    if (rc)
        return rc;
    ctx->list_pool_cap = words;
    ctx->T->grids_built_for[0] = -1; // the next trt_set_scene / table setter builds again
    return TRT_OK;
}

extern "C" int trt_read_diagnostics(trt_context *ctx, unsigned long long *wave_loop_trips, unsigned long long *phase2_rounds)
{
    if (!ctx)
        return fail(TRT_ERR_ARGUMENT, "ctx is NULL");
    if (wave_loop_trips)
        *wave_loop_trips = ctx->last_trips;
    if (phase2_rounds)
        *phase2_rounds = ctx->last_phase2;
    return TRT_OK;
}

extern "C" int trt_read_sweep_fallbacks(trt_context *ctx, unsigned long long *swept_traces)
{
    if (!ctx || !swept_traces)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    *swept_traces = ctx->last_swept;
    return TRT_OK;
}

extern "C" int trt_read_loop_diagnostics(trt_context *ctx, unsigned long long out[8])
{
    if (!ctx || !out)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    memcpy(out, ctx->last_loops, sizeof ctx->last_loops);
    return TRT_OK;
}

extern "C" int trt_read_shading_passes(trt_context *ctx, unsigned long long *passes)
{
    if (!ctx || !passes)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    *passes = ctx->last_passes;
    return TRT_OK;
}

extern "C" int trt_path_family_code(trt_context *ctx, int kind, int sphere, const double *parent_origin)
{
    if (!ctx || !ctx->have_scene || !ctx->grids.path_enabled || kind < 0 || kind > 3)
        return -1;
    if (kind < 2)
        return kind;
    const int n = (int)(ctx->T->h_spheres.size() / 9);
    if (sphere < 0 || sphere >= n)
        return -1;
    if (kind == 2)
        return 2 + sphere;
    if (!parent_origin)
        return -1;
    if (!ctx->grids.patch_m)
        return 2 + n + sphere; // one family per sphere
    const double *c = ctx->T->h_spheres.data() + 9 * (size_t)sphere;
    const int k = trt_patch_of(ctx->grids.patch_m, parent_origin[0] - c[0], parent_origin[1] - c[1], parent_origin[2] - c[2]);
    return 2 + n + ((sphere << TRT_PATCH_SHIFT) | k);
}

extern "C" long trt_read_path_tables(trt_context *ctx, const Camera *camera, unsigned long long *cells, size_t capacity_cells,
                                     unsigned long long *pool, size_t capacity_pool, long info[8])
{
    if (!ctx || !camera || !cells || !pool || !info)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "no scene");
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ensure_eye_tables(ctx, camera, ctx->stream);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const trt::GridView &g = ctx->grids;
    const int n = (int)(ctx->T->h_spheres.size() / 9);
    unsigned long long used[16 * (1 + kEyeSlots)] = {0};
    HIP_TRY(hipMemcpy(used, ctx->T->d_pool_used.ptr, sizeof used, hipMemcpyDeviceToHost));
    const size_t eye_total = 2 * 6 * (size_t)g.g_eye * g.g_eye, sph_total = 2 * (size_t)n * (size_t)g.patch_count * 6 * (size_t)g.g_sph * g.g_sph;
    const size_t total = g.path_enabled ? eye_total + sph_total : 0;
    const size_t pool_words = ctx->T->pool_scene_words + kEyeSlots * ctx->T->pool_eye_words; // the whole pool: the cells' offsets are into it
    const size_t eye_from = ctx->T->pool_scene_words + (size_t)ctx->eye_slot * ctx->T->pool_eye_words;
    info[0] = g.path_enabled, info[1] = g.g_eye, info[2] = g.g_sph, info[3] = n, info[4] = (long)total;
    info[5] = (long)std::min<unsigned long long>(used[0], 1ull << 62), info[6] = (long)used[16 * (1 + ctx->eye_slot)] - (long)eye_from, info[7] = (long)pool_words;
    if (!g.path_enabled)
        return 0;
    if (capacity_cells < total || capacity_pool < pool_words)
        return fail(TRT_ERR_CAPACITY, "tables have %zu cells and %zu pool words", total, pool_words);
    HIP_TRY(hipMemcpy(cells, ctx->T->d_path_lists.ptr + g.eye_at, eye_total * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (sph_total)
        HIP_TRY(hipMemcpy(cells + eye_total, ctx->T->d_path_lists.ptr + g.sph_at, sph_total * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pool, ctx->T->d_pool.ptr, pool_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (long)total;
}

extern "C" long trt_read_path_lean_tables(trt_context *ctx, unsigned long long *cells, size_t capacity_cells)
{
    if (!ctx || !cells)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "no scene");
    const trt::GridView &g = ctx->grids;
    if (!g.path_enabled || !ctx->T->lean_at)
        return 0;
    const size_t total = ctx->T->h_spheres.size() / 9 * (size_t)g.patch_count * 6 * (size_t)g.g_sph * g.g_sph;
    if (capacity_cells < total)
        return fail(TRT_ERR_CAPACITY, "the twins have %zu cells", total);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (total)
        HIP_TRY(hipMemcpy(cells, ctx->T->d_path_lists.ptr + ctx->T->lean_at, total * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (long)total;
}

extern "C" long trt_read_light_grid(trt_context *ctx, int point_light, int index, unsigned long long *masks, size_t capacity_words)
{
    if (!ctx || !masks || index < 0)
        return fail(TRT_ERR_ARGUMENT, "bad argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "no scene");
    const trt::GridView &g = ctx->grids;
    if (!g.enabled)
        return 0;
    if (index >= (point_light ? ctx->scene.num_point : ctx->scene.num_dir))
        return fail(TRT_ERR_ARGUMENT, "light %d", index);
    const size_t words = (size_t)std::max((ctx->scene.num_spheres + 63) / 64, 1);
    const size_t stride = (point_light ? g.point_stride : g.dir_stride) * words; // mask words of one light's table
    if (capacity_words < stride)
        return fail(TRT_ERR_CAPACITY, "table has %zu words, buffer %zu", stride, capacity_words);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(masks, (point_light ? ctx->T->d_point_masks.ptr : ctx->T->d_dir_masks.ptr) + stride * (size_t)index, stride * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    return (long)stride;
}

extern "C" long trt_read_light_lists(trt_context *ctx, int point_light, int index, unsigned long long *cells, size_t capacity_cells,
                                     unsigned long long *pool, size_t capacity_pool, long info[4])
{
    const bool query = !cells && !pool && !capacity_cells && !capacity_pool; // sizes only: info is filled, nothing is copied
    if (!ctx || !info || index < 0 || (!query && (!cells || !pool)))
        return fail(TRT_ERR_ARGUMENT, "bad argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "no scene");
    const trt::GridView &g = ctx->grids;
    const size_t stride = point_light ? g.point_stride : g.dir_stride; // list cells of one light's table
    const size_t pool_words = ctx->T->pool_scene_words;                // the light tables' long lists live in the scene's part
    info[0] = g.enabled ? (long)stride : 0, info[1] = g.list_bits, info[2] = g.enabled ? (long)pool_words : 0, info[3] = g.enabled;
    if (!g.enabled)
        return 0;
    if (index >= (point_light ? ctx->scene.num_point : ctx->scene.num_dir))
        return fail(TRT_ERR_ARGUMENT, "light %d", index);
    if (query)
        return (long)stride;
    if (capacity_cells < stride || capacity_pool < pool_words)
        return fail(TRT_ERR_CAPACITY, "table has %zu cells and %zu pool words", stride, pool_words);
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(cells, (point_light ? ctx->T->d_point_lists.ptr : ctx->T->d_dir_lists.ptr) + stride * (size_t)index, stride * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pool, ctx->T->d_pool.ptr, pool_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return (long)stride;
}

extern "C" int trt_selftest_div_sqrt(trt_context *ctx, const double *a, const double *b, size_t n, double *quot, double *root)
{
    if (!ctx || !a || !b || !quot || !root)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceBuffer<double> buf;
    HIP_TRY(buf.reserve(4 * n));
    double *da = buf.ptr, *db = buf.ptr + n, *dq = buf.ptr + 2 * n, *dr = buf.ptr + 3 * n;
    HIP_TRY(hipMemcpy(da, a, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b, n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(trt::div_sqrt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, da, db, (long)n, dq, dr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(quot, dq, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(root, dr, n * sizeof(double), hipMemcpyDeviceToHost));
    return TRT_OK;
}

extern "C" int trt_selftest_unit(trt_context *ctx, const double *xyzw, size_t n, double *fast, double *reference)
{
    if (!ctx || !xyzw || !fast || !reference)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceBuffer<double> buf;
    HIP_TRY(buf.reserve(12 * n));
    double *dv = buf.ptr, *df = buf.ptr + 4 * n, *dr = buf.ptr + 8 * n;
    HIP_TRY(hipMemcpy(dv, xyzw, 4 * n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(trt::unit_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, dv, (long)n, df, dr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(fast, df, 4 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(reference, dr, 4 * n * sizeof(double), hipMemcpyDeviceToHost));
    return TRT_OK;
}

namespace
{
// trt_cube_lookup as the DEVICE evaluates it (v_cubeid / v_cubesc / v_cubetc / v_cubema): {face, sc, tc, ma2} per direction
__global__ void cube_selftest_kernel(const float *xyz, long n, float *out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    int face;
    float sc, tc, ma2;
    trt_cube_lookup(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &face, &sc, &tc, &ma2);
    out[4 * i] = (float)face, out[4 * i + 1] = sc, out[4 * i + 2] = tc, out[4 * i + 3] = ma2;
}
} // namespace

namespace
{
// trt_selftest_sky: per direction the reference's texel index by the FP64 form, the FP32 estimate's, and whether the estimate
// calls itself ambiguous (the kernel then takes the FP64 form)
__global__ void sky_selftest_kernel(const double *dirs, long n, int dim, long *exact, long *estimate, int *ambiguous)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const trt::d3 d = trt::d3{dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]};
    bool amb;
    exact[i] = trt::sky_index_unit(dim, d, (double)dim);
    estimate[i] = trt::sky_index_estimate(dim, (float)dim, d, amb);
    ambiguous[i] = amb;
}
} // namespace

extern "C" int trt_selftest_sky(trt_context *ctx, const double *dirs, size_t n, int dim, long long *exact, long long *estimate, int *ambiguous)
{
    if (!ctx || !dirs || !exact || !estimate || !ambiguous || dim < 1)
        return fail(TRT_ERR_ARGUMENT, "bad argument");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceBuffer<double> in;
    DeviceBuffer<long> out;
    DeviceBuffer<int> flags;
    HIP_TRY(in.reserve(3 * n));
    HIP_TRY(out.reserve(2 * n));
    HIP_TRY(flags.reserve(n));
    HIP_TRY(hipMemcpy(in.ptr, dirs, 3 * n * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sky_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)in.ptr, (long)n, dim, out.ptr, out.ptr + n, flags.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(exact, out.ptr, n * sizeof(long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(estimate, out.ptr + n, n * sizeof(long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ambiguous, flags.ptr, n * sizeof(int), hipMemcpyDeviceToHost));
    return TRT_OK;
}

extern "C" int trt_selftest_cube(trt_context *ctx, const float *xyz, size_t n, float *device_out, float *host_out)
{
    if (!ctx || !xyz || !device_out || !host_out)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceBuffer<float> buf;
    HIP_TRY(buf.reserve(7 * n));
    HIP_TRY(hipMemcpy(buf.ptr, xyz, 3 * n * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(cube_selftest_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (const float *)buf.ptr, (long)n, buf.ptr + 3 * n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(device_out, buf.ptr + 3 * n, 4 * n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
    { // the same header compiled for the host: the C restatement of the four instructions
        int face;
        float sc, tc, ma2;
        trt_cube_lookup(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], &face, &sc, &tc, &ma2);
        host_out[4 * i] = (float)face, host_out[4 * i + 1] = sc, host_out[4 * i + 2] = tc, host_out[4 * i + 3] = ma2;
    }
    return TRT_OK;
}

extern "C" int trt_probe_rays(trt_context *ctx, const Ray *rays, size_t n, int *obj, double *point, double *normal,
                              double *material, double *lit)
{
    if (!ctx || !rays || !obj || !point || !normal || !material || !lit)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "trt_set_scene has not been called");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    DeviceBuffer<double> buf;
    DeviceBuffer<int> dobj;
    HIP_TRY(buf.reserve(n * (6 + 3 + 3 + 5 + 3)));
    HIP_TRY(dobj.reserve(n));
    double *dr = buf.ptr, *dp = dr + 6 * n, *dn = dp + 3 * n, *dm = dn + 3 * n, *dl = dm + 5 * n;
    HIP_TRY(hipMemcpy(dr, rays, n * sizeof(Ray), hipMemcpyHostToDevice));
    // the context's switches: the specular extension, or the sky filter (trt_set_sky_filter); both together no render accepts, and the
    // specular one goes first here
    const auto probe = ctx->specular ? trt::probe_rays_kernel<true> : ctx->sky_filter ? trt::probe_rays_kernel<false, true> : trt::probe_rays_kernel<false>;
    hipLaunchKernelGGL(probe, dim3((unsigned)((n + 255) / 256)), dim3(256),
                       scene_lds_bytes(ctx->scene), ctx->stream, ctx->scene, (const double *)dr, (long)n, dobj.ptr, dp, dn, dm, dl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(obj, dobj.ptr, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(point, dp, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(normal, dn, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(material, dm, 5 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lit, dl, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    return TRT_OK;
}

// only codes the kernel can decode reach it: 0, 1, 2 + i, and 2 + N + i (one family per sphere) or 2 + N + (i << 7 | k) with
// k < patches (a patch number beyond the tables would index past the LDS image and the lists); anything else: no family
static std::vector<int> decodable_family_codes(const trt_context *ctx, const int *families, size_t n)
{
    const int ns = ctx->scene.num_spheres, pm = ctx->grids.path_enabled ? ctx->grids.patch_m : 0, pc = ctx->grids.path_enabled ? ctx->grids.patch_count : 0;
    std::vector<int> codes(families, families + n);
    for (int &c : codes)
    {
        bool ok = c == 0 || c == 1 || (c >= 2 && c < 2 + ns);
        if (!ok && c >= 2 + ns)
        {
            const int rest = c - 2 - ns;
            ok = pm ? ((rest >> TRT_PATCH_SHIFT) < ns && (rest & ((1 << TRT_PATCH_SHIFT) - 1)) < pc) : rest < ns;
        }
        if (!ok)
            c = -1;
    }
    return codes;
}

extern "C" int trt_probe_rays_production(trt_context *ctx, const Camera *camera, const Ray *rays, const int *families, size_t n, int *obj,
                                         double *point, double *normal, double *material, double *lit)
{
    if (!ctx || !camera || !rays || !obj || !point || !normal || !material || !lit)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "trt_set_scene has not been called");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc = ensure_eye_tables(ctx, camera, ctx->stream);
    if (rc)
        return rc;
    DeviceBuffer<double> buf;
    DeviceBuffer<int> dobj;
    HIP_TRY(buf.reserve(n * (6 + 3 + 3 + 5 + 3)));
    HIP_TRY(dobj.reserve(2 * n));
    double *dr = buf.ptr, *dp = dr + 6 * n, *dn = dp + 3 * n, *dm = dn + 3 * n, *dl = dm + 5 * n;
    HIP_TRY(hipMemcpy(dr, rays, n * sizeof(Ray), hipMemcpyHostToDevice));
    if (families)
    {
        const std::vector<int> codes = decodable_family_codes(ctx, families, n);
        HIP_TRY(hipMemcpy(dobj.ptr + n, codes.data(), n * sizeof(int), hipMemcpyHostToDevice));
    }
    trt::FrameView f{};
    memcpy(f.cam, camera, sizeof(Camera));
    f.jitter = ctx->d_jitter.ptr; // spp = 0: nothing is read through it
    const bool patches = ctx->grids.path_enabled && ctx->grids.patch_m > 0;
    const auto probe = patches ? (ctx->specular ? trt::probe_rounds_kernel<true, true> : ctx->sky_filter ? trt::probe_rounds_kernel<true, false, true> : trt::probe_rounds_kernel<true>)
                               : (ctx->specular ? trt::probe_rounds_kernel<false, true> : ctx->sky_filter ? trt::probe_rounds_kernel<false, false, true> : trt::probe_rounds_kernel<false>); // trt_set_specular, trt_set_sky_filter
    hipLaunchKernelGGL(probe, dim3((unsigned)((n + trt::kPersistentBlock - 1) / trt::kPersistentBlock)), dim3(trt::kPersistentBlock),
                       image_lds_bytes(ctx, 0), ctx->stream, ctx->scene, ctx->cull, f, ctx->grids, (const double *)dr,
                       families ? (const int *)(dobj.ptr + n) : (const int *)nullptr, (long)n, dobj.ptr, dp, dn, dm, dl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(obj, dobj.ptr, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(point, dp, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(normal, dn, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(material, dm, 5 * n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(lit, dl, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    return TRT_OK;
}

// ---- where the device looks: trt_probe_path_lookups, trt_probe_shadow_lookups, trt_selftest_filter ----------------------------

namespace trt
{
namespace
{
struct PathLookupIo
{
    const double *rays;
    const int *families, *frames;
    long count;
    int *fallback, *successor;
    unsigned long long *word;
    long long *read_at;
};

// one lane per ray through the render kernels' own look-up, with its diagnostic output switched on
template <bool PATCHES, bool BATCH>
TRT_DEV void path_lookup_lane(const LdsImage &L, const GridView &grids, int n, const PathLookupIo &io)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = i < io.count;
    const long at = alive ? i : 0;
    const d3 o = load3(io.rays + 6 * at), d = load3(io.rays + 6 * at + 3);
    int fam = io.families[at];
    const int frame = BATCH ? io.frames[at] : 0;
    unsigned long long fallback_lanes = 0, cell;
    long long read_at = -1;
    if constexpr (PATCHES)
        cell = path_cell_patches<BATCH, true>(L, grids, n, fam, o, d, alive, lanes_with(alive), fallback_lanes, frame, -1, &read_at);
    else
        cell = path_cell<BATCH, true>(L, grids, n, fam, o, d, alive, lanes_with(alive), fallback_lanes, frame, -1, &read_at);
    if (!alive)
        return;
    io.fallback[i] = (int)((fallback_lanes >> (threadIdx.x & 63)) & 1);
    io.word[i] = cell;
    io.successor[i] = fam;
    io.read_at[i] = read_at;
}

template <bool PATCHES>
__global__ __launch_bounds__(kPersistentBlock) void path_lookup_kernel(SceneView s, CullView cull, FrameView f, GridView grids, PathLookupIo io)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const LdsImage L = stage_lds_image(lds, s, cull, f, grids);
    path_lookup_lane<PATCHES, false>(L, grids, s.num_spheres, io);
}

// the first five arguments are a BATCH launch's: stage_lds_image_batch reads the fifth from the kernarg segment at kArgBatch
template <bool PATCHES>
__global__ __launch_bounds__(kPersistentBlock) void path_lookup_batch_kernel(SceneView s, CullView cull, FrameView f, GridView grids, BatchView batch, PathLookupIo io)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const LdsImage L = stage_lds_image_batch(lds, s, cull, f, grids);
    path_lookup_lane<PATCHES, true>(L, grids, s.num_spheres, io);
}
static_assert(kArgBatch + sizeof(BatchView) + sizeof(PathLookupIo) <= 4096, "the look-up probe's arguments fit the kernarg segment");

struct ShadowLookupIo
{
    const double *origins;
    long count;
    int light, pad_;
    int *far, *cell;
    unsigned long long *word;
    double *lo, *hi;
};

// shadow_stage's look-up lines for light `io.light` (the same for every lane), on the staged headers
__global__ __launch_bounds__(kPersistentBlock) void shadow_lookup_kernel(SceneView s, CullView cull, FrameView f, GridView grids, ShadowLookupIo io)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const LdsImage L = stage_lds_image(lds, s, cull, f, grids);
    const int nd = s.num_dir, li = io.light;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = i < io.count;
    const long at = alive ? i : 0;
    const d3 o = load3(io.origins + 3 * at);
    int far = 1, c = -1;
    unsigned long long cell = 0;
    double lo = 0.0, hi = 0.0;
    if (li < nd)
    {
        const trt_dirgrid *G = L.dirgrid + li;
        c = trt_dirgrid_cell(G, o.x, o.y, o.z, &far);
        if (alive && !far && (unsigned)c < grids.dir_stride) // the bound: this probe must not fault where a look-up went astray
            cell = grids.dir_lists[(size_t)li * grids.dir_stride + (unsigned)c];
    }
    else
    {
        const double *pl = L.pt + (li - nd) * 7;
        const d3 to_light = sub(load3(pl), o);
        const double light_d2 = dot(to_light, to_light);
        const d3 sd = unit(to_light);
        const trt_pointgrid *G = L.pointgrid + (li - nd);
        c = trt_pointgrid_cell(G, o.x, o.y, o.z, &far);
        far |= !(__builtin_fabs(dot(sd, sd) - 1.0) <= 9.094947017729282e-13);
        if (alive && !far && (unsigned)c < grids.point_stride)
            cell = grids.point_lists[(size_t)(li - nd) * grids.point_stride + (unsigned)c];
        trt_point_shadow_bounds(G, light_d2, dot(sd, sd), &lo, &hi);
    }
    if (!alive)
        return;
    io.far[i] = far;
    io.cell[i] = c;
    io.word[i] = cell;
    if (io.lo)
        io.lo[i] = lo, io.hi[i] = hi;
}

struct FilterIo
{
    const double *rays;
    long count;
    unsigned *fields, *sign, *sign_fixed;
};

__global__ __launch_bounds__(kPersistentBlock) void filter_selftest_kernel(SceneView s, CullView cull, FrameView f, GridView grids, FilterIo io)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const LdsImage L = stage_lds_image(lds, s, cull, f, grids);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= io.count)
        return;
    const d3 o = load3(io.rays + 6 * i), d = load3(io.rays + 6 * i + 3);
    trt_ray_filter flt;
    trt_filter_setup(&flt, o.x, o.y, o.z, d.x, d.y, d.z, dot(d, d), cull.c0x, cull.c0y, cull.c0z, cull.cn, cull.rm); // as trace() sets it up
    const float fields[8] = {flt.dx, flt.dy, flt.dz, flt.wx, flt.wy, flt.wz, flt.neg_thr, flt.cd_min};
    for (int k = 0; k < 8; k++)
        io.fields[9 * i + k] = __builtin_bit_cast(unsigned, fields[k]);
    io.fields[9 * i + 8] = (unsigned)flt.ok;
    for (int j = 0; j < s.num_spheres; j++)
    {
        const float4 e = L.cull[j];
        io.sign[(size_t)j * (size_t)io.count + (size_t)i] = trt_filter_sign(&flt, e.x, e.y, e.z, e.w);
    }
    if (io.sign_fixed)
        for (int j = 0; j < s.num_spheres; j++)
        {
            const float4 e = L.cull_dir[j]; // the row of directional light 0
            io.sign_fixed[(size_t)j * (size_t)io.count + (size_t)i] = trt_filter_sign_fixed_dir(&flt, e.x, e.y, e.z, e.w);
        }
}
} // namespace
} // namespace trt

namespace trt_impl
{
void allow_large_lds_lookups(const trt_context *ctx)
{
    (void)hipFuncSetAttribute((const void *)trt::path_lookup_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::path_lookup_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::path_lookup_batch_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::path_lookup_batch_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::shadow_lookup_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
    (void)hipFuncSetAttribute((const void *)trt::filter_selftest_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ctx->lds_limit);
}

// a probe's image must fit LDS like a frame's (the probes have no device-memory form)
static int lookup_lds_bytes(const trt_context *ctx, int frames, size_t *bytes)
{
    *bytes = image_lds_bytes(ctx, 0, frames);
    if (*bytes > (size_t)ctx->lds_limit)
        return fail(TRT_ERR_CAPACITY, "the scene image (%zu bytes) does not fit LDS (%d)", *bytes, ctx->lds_limit);
    allow_large_lds_lookups(ctx);
    return TRT_OK;
}

// {region, table, cell} of an index into the path rays' list cells, from where the context's tables lie (GridView) and nothing else
static void place_of_read(const trt_context *ctx, long long at, int place[3])
{
    const trt::GridView &g = ctx->grids;
    const long long eye_cells = 6LL * g.g_eye * g.g_eye, sph_cells = 6LL * g.g_sph * g.g_sph;
    const long long tables = 2LL * ctx->scene.num_spheres * g.patch_count;
    const long long sph_from = g.sph_at, sph_to = sph_from + tables * sph_cells;
    const long long lean_from = g.lean_off ? sph_from + (long long)g.lean_off : -1, lean_to = lean_from + tables / 2 * sph_cells;
    place[0] = -2, place[1] = place[2] = -1;
    if (at < 0)
        place[0] = -1;
    else if (at < sph_from) // kEyeSlots slots of two tables
        place[0] = 0, place[1] = (int)(at / eye_cells), place[2] = (int)(at % eye_cells);
    else if (at < sph_to)
        place[0] = 1, place[1] = (int)((at - sph_from) / sph_cells), place[2] = (int)((at - sph_from) % sph_cells);
    else if (lean_from >= 0 && at >= lean_from && at < lean_to)
        place[0] = 2, place[1] = (int)((at - lean_from) / sph_cells), place[2] = (int)((at - lean_from) % sph_cells);
}
} // namespace trt_impl

extern "C" int trt_probe_path_lookups(trt_context *ctx, const Camera *cameras, int n_cameras, const Ray *rays, const int *families, const int *frames, size_t n,
                                      int *fallback, unsigned long long *cell_word, int *successor, long long *read_at, int *place)
{
    if (!ctx || !cameras || !rays || !families || !fallback || !cell_word || !successor || !read_at || !place)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (n_cameras < 1 || n_cameras > TRT_BATCH_MAX)
        return fail(TRT_ERR_ARGUMENT, "1 to %d cameras, %d given", TRT_BATCH_MAX, n_cameras);
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "trt_set_scene has not been called");
    if (!ctx->grids.path_enabled)
        return fail(TRT_ERR_ARGUMENT, "the scene has no path tables: nothing is looked up");
    if (n_cameras > 1 && ctx->T.use_count() > 1)
        return fail(TRT_ERR_CAPACITY, "a batch builds its eye tables in slots that belong to the contexts this one shares its scene with");
    if (n == 0)
        return TRT_OK;
    for (size_t i = 0; frames && i < n; i++)
        if (frames[i] < 0 || frames[i] >= n_cameras)
            return fail(TRT_ERR_ARGUMENT, "frames[%zu] = %d of %d cameras", i, frames[i], n_cameras);
    HIP_TRY(hipSetDevice(ctx->device));
    const bool batch = n_cameras > 1;
    size_t lds = 0;
    int rc = lookup_lds_bytes(ctx, n_cameras, &lds);
    if (rc)
        return rc;
    for (int b = 0; b < n_cameras; b++) // as a frame does: the single camera in the context's own slot, frame b of a batch in slot b
    {
        rc = ensure_eye_tables(ctx, &cameras[b], ctx->stream, batch ? b : -1);
        if (rc)
            return rc;
    }
    const std::vector<int> codes = decodable_family_codes(ctx, families, n);
    const std::vector<int> zero_frames(frames ? 0 : n, 0);
    DeviceBuffer<double> d_rays;
    DeviceBuffer<int> d_int;
    DeviceBuffer<unsigned long long> d_word;
    HIP_TRY(d_rays.reserve(6 * n));
    HIP_TRY(d_int.reserve(4 * n));
    HIP_TRY(d_word.reserve(2 * n));
    HIP_TRY(hipMemcpy(d_rays.ptr, rays, n * sizeof(Ray), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_int.ptr, codes.data(), n * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_int.ptr + n, frames ? frames : zero_frames.data(), n * sizeof(int), hipMemcpyHostToDevice));
    trt::PathLookupIo io{d_rays.ptr, d_int.ptr, d_int.ptr + n, (long)n, d_int.ptr + 2 * n, d_int.ptr + 3 * n, d_word.ptr, (long long *)(d_word.ptr + n)};
    trt::FrameView f{};
    memcpy(f.cam, &cameras[0], sizeof(Camera));
    f.jitter = ctx->d_jitter.ptr; // spp = 0: nothing is read through it
    const bool patches = ctx->grids.patch_m > 0;
    const dim3 grid((unsigned)((n + trt::kPersistentBlock - 1) / trt::kPersistentBlock)), block(trt::kPersistentBlock);
    if (!batch)
    {
        if (patches)
            hipLaunchKernelGGL(trt::path_lookup_kernel<true>, grid, block, lds, ctx->stream, ctx->scene, ctx->cull, f, ctx->grids, io);
        else
            hipLaunchKernelGGL(trt::path_lookup_kernel<false>, grid, block, lds, ctx->stream, ctx->scene, ctx->cull, f, ctx->grids, io);
    }
    else
    { // the arguments of a batch launch (trt_render.hip: render_device_batch): frame b reads eye slot b
        trt::GridView g = ctx->grids;
        g.eye_at = 0;
        trt::BatchView view{};
        for (int b = 0; b < n_cameras; b++)
        {
            memcpy(view.cam[b], &cameras[b], sizeof(Camera));
            view.eye[b][0] = ctx->eye_slots[b].families[0], view.eye[b][1] = ctx->eye_slots[b].families[1];
        }
        g.eye[0] = view.eye[0][0], g.eye[1] = view.eye[0][1];
        view.frames = (unsigned)n_cameras;
        view.units_per_frame = 1, view.frame_magic = 0xffffffffu; // the hand-out's: not read here
        if (patches)
            hipLaunchKernelGGL(trt::path_lookup_batch_kernel<true>, grid, block, lds, ctx->stream, ctx->scene, ctx->cull, f, g, view, io);
        else
            hipLaunchKernelGGL(trt::path_lookup_batch_kernel<false>, grid, block, lds, ctx->stream, ctx->scene, ctx->cull, f, g, view, io);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(fallback, d_int.ptr + 2 * n, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(successor, d_int.ptr + 3 * n, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cell_word, d_word.ptr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(read_at, d_word.ptr + n, n * sizeof(long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++)
        place_of_read(ctx, read_at[i], place + 3 * i);
    return TRT_OK;
}

extern "C" int trt_probe_shadow_lookups(trt_context *ctx, const double *origins, size_t n, int light, int *far, int *cell, unsigned long long *cell_word,
                                        double *lo, double *hi)
{
    if (!ctx || !origins || !far || !cell || !cell_word || (!lo) != (!hi))
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "trt_set_scene has not been called");
    if (!ctx->grids.enabled)
        return fail(TRT_ERR_ARGUMENT, "the scene has no light tables: nothing is looked up");
    if (light < 0 || light >= ctx->scene.num_dir + ctx->scene.num_point)
        return fail(TRT_ERR_ARGUMENT, "light %d of %d", light, ctx->scene.num_dir + ctx->scene.num_point);
    if (light >= ctx->scene.num_dir && !lo)
        return fail(TRT_ERR_ARGUMENT, "a point light's look-up returns lo and hi");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    size_t lds = 0;
    const int rc = lookup_lds_bytes(ctx, 1, &lds);
    if (rc)
        return rc;
    DeviceBuffer<double> d_real;
    DeviceBuffer<int> d_int;
    DeviceBuffer<unsigned long long> d_word;
    HIP_TRY(d_real.reserve(5 * n));
    HIP_TRY(d_int.reserve(2 * n));
    HIP_TRY(d_word.reserve(n));
    HIP_TRY(hipMemcpy(d_real.ptr, origins, 3 * n * sizeof(double), hipMemcpyHostToDevice));
    trt::ShadowLookupIo io{d_real.ptr, (long)n, light, 0, d_int.ptr, d_int.ptr + n, d_word.ptr, lo ? d_real.ptr + 3 * n : nullptr, lo ? d_real.ptr + 4 * n : nullptr};
    trt::FrameView f{};
    f.jitter = ctx->d_jitter.ptr; // spp = 0: nothing is read through it
    hipLaunchKernelGGL(trt::shadow_lookup_kernel, dim3((unsigned)((n + trt::kPersistentBlock - 1) / trt::kPersistentBlock)), dim3(trt::kPersistentBlock), lds, ctx->stream,
                       ctx->scene, ctx->cull, f, ctx->grids, io);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(far, d_int.ptr, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cell, d_int.ptr + n, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(cell_word, d_word.ptr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (lo)
    {
        HIP_TRY(hipMemcpy(lo, d_real.ptr + 3 * n, n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(hi, d_real.ptr + 4 * n, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return TRT_OK;
}

extern "C" int trt_selftest_filter(trt_context *ctx, const Ray *rays, size_t n, unsigned *fields, unsigned *sign, unsigned *sign_fixed)
{
    if (!ctx || !rays || !fields || !sign)
        return fail(TRT_ERR_ARGUMENT, "NULL argument");
    if (!ctx->have_scene)
        return fail(TRT_ERR_NO_SCENE, "trt_set_scene has not been called");
    if (sign_fixed && ctx->scene.num_dir < 1)
        return fail(TRT_ERR_ARGUMENT, "the scene has no directional light: there is no fixed-direction table");
    if (n == 0)
        return TRT_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    size_t lds = 0;
    const int rc = lookup_lds_bytes(ctx, 1, &lds);
    if (rc)
        return rc;
    const size_t ns = (size_t)ctx->scene.num_spheres;
    DeviceBuffer<double> d_rays;
    DeviceBuffer<unsigned> d_out;
    HIP_TRY(d_rays.reserve(6 * n));
    HIP_TRY(d_out.reserve(std::max<size_t>(n * (9 + 2 * ns), 1)));
    HIP_TRY(hipMemcpy(d_rays.ptr, rays, n * sizeof(Ray), hipMemcpyHostToDevice));
    unsigned *const d_sign = d_out.ptr + 9 * n, *const d_fixed = d_sign + ns * n;
    trt::FilterIo io{d_rays.ptr, (long)n, d_out.ptr, d_sign, sign_fixed ? d_fixed : nullptr};
    trt::FrameView f{};
    f.jitter = ctx->d_jitter.ptr; // spp = 0: nothing is read through it
    hipLaunchKernelGGL(trt::filter_selftest_kernel, dim3((unsigned)((n + trt::kPersistentBlock - 1) / trt::kPersistentBlock)), dim3(trt::kPersistentBlock), lds, ctx->stream,
                       ctx->scene, ctx->cull, f, ctx->grids, io);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    HIP_TRY(hipMemcpy(fields, d_out.ptr, 9 * n * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (ns)
    {
        HIP_TRY(hipMemcpy(sign, d_sign, ns * n * sizeof(unsigned), hipMemcpyDeviceToHost));
        if (sign_fixed)
            HIP_TRY(hipMemcpy(sign_fixed, d_fixed, ns * n * sizeof(unsigned), hipMemcpyDeviceToHost));
    }
    return TRT_OK;
}

// ---- default context: the drop-in layer ---------------------------------------------------------------------

