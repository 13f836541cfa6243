/*
 * trt_hip_diag.h -- DIAGNOSTIC and TEST entries of libtrt_hip.so.  Not part of the drop-in boundary (include/trt_hip.h): nothing
 * here is needed to produce a frame, a maintainer of the reference would not bind any of it, and any of it may change with the
 * kernels.  Used by tests/, bench.py (ray counts, loop diagnostics) and tools/.
 *
 *   counters      trace_ray calls of the last frame as the kernel counted them (the metric's numerator), loop diagnostics
 *   read-backs    the candidate tables the device built, for comparison with the host reference builders
 *   self-tests    device division / square root / normalisation / cube instructions / skybox estimate against their references
 *   probes        single rays through the reference-order kernel and through the production kernel's stages
 *   look-ups      where the kernels' own table look-ups and the FP32 filter look, for the host's conservativeness checks
 *   scene image   where the kernels read the scene from: LDS or device memory
 *   drop-in       a borrowed handle to the default context; how many table builds and skybox uploads a context has performed
 *   test hooks    the pool cap of the long candidate lists; a NaN fill of a launch's scratch and output; a stand-in for RCCL so that several ranks can share one GPU
 */
#ifndef TRT_HIP_DIAG_H
#define TRT_HIP_DIAG_H

#include "trt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tests: cap the scene's part of the pool of long candidate lists, and the part of every eye slot (the eye's two tables are
 * rebuilt per camera into a part of their own), at `words` 64-bit words (0 = automatic) from the next trt_set_scene on; lists
 * that find no room leave their cell without a list and its rays sweep -- frames stay bit-identical. */
int trt_set_list_pool_words(trt_context *ctx, size_t words);

/* Work counters of the LAST rendered frame (device atomics, only when enabled; off by default
 * so timed runs carry no atomics).  path = trace calls from the bounce loop (TRT.c:1024),
 * shadow = trace calls from lighting (TRT.c:907, :937). */
int trt_enable_counters(trt_context *ctx, int enable);

int trt_read_counters(trt_context *ctx, unsigned long long *path_rays, unsigned long long *shadow_rays);

/* Diagnostics of the last counted frame (valid after trt_read_counters, production kernel only):
 * iterations of the per-wave main loop summed over waves, and exact-test (phase 2) rounds.
 * Lane utilisation of the trace loop = (path + shadow) / (64 * wave_loop_trips). */
int trt_read_diagnostics(trt_context *ctx, unsigned long long *wave_loop_trips, unsigned long long *phase2_rounds);

/* The family code of the production kernel for a path ray (trt_probe_rays_production): kind 0 = the ray starts at the eye,
 * 1 = reflected by the ground, parent from the eye, 2 = the ray starts on `sphere`, 3 = reflected by the ground, its parent
 * started on `sphere` at parent_origin (3 doubles: the patch of the sphere follows from it).  -1: no family. */
int trt_path_family_code(trt_context *ctx, int kind, int sphere, const double *parent_origin);

/* Copy the path rays' tables to the host (tests: the device-built lists must equal the host reference builder's): list
 * cells (2*6*eye_cells^2, then 2NP*6*sphere_cells^2 for P patches per sphere: patch k of sphere i at i P + k, then the mirror
 * images in the same order) and the pool of long lists, as built for `camera`'s eye.
 * info: {enabled, eye_cells, sphere_cells, N, cells, pool words used by the scene's tables, by the eye's, pool capacity}.
 * Returns the number of cells copied, 0 when the tables are off, or a negative TRT_ERR_*. */
long trt_read_path_tables(trt_context *ctx, const Camera *camera, unsigned long long *cells, size_t capacity_cells,
                          unsigned long long *pool, size_t capacity_pool, long info[8]);

/* LEAN TWINS of the spheres' own families (csrc/trt_raygrid.h): a path ray that leaves sphere i outwards, (o - c_i).d >= 0 as the
 * exact test itself forms it, reads its cell's list without entry i -- that test would answer "miss".  mode 1: on (the twins are
 * built if the scene has none; not on tables shared with other contexts), 0: every look-up reads the full tables, exactly as
 * without twins, -1 (default): on where tables and twins together stay within the budget that chooses the patches
 * (trt_set_path_patches), and not for a scene that changes from call to call.  Frames and ray counts do not depend on it.
 * Environment TRT_PATH_LEAN sets the default.  The getter: whether the next frame reads twins, and the bytes they take (part of
 * trt_scene_info's table_bytes). */
int trt_set_path_lean_lists(trt_context *ctx, int mode);
int trt_get_path_lean_lists(trt_context *ctx, int *in_use, unsigned long long *twin_bytes);
/* The twins' cells (N P * 6 * sphere_cells^2, in the order of the non-mirrored tables of trt_read_path_tables, whose pool their
 * long lists point into).  Returns the number of cells copied, 0 when the scene has no twins, or a negative TRT_ERR_*. */
long trt_read_path_lean_tables(trt_context *ctx, unsigned long long *cells, size_t capacity_cells);

/* After trt_read_counters: the number of wave-level traces of the last counted frame in which some ray failed its table's
 * membership / range test and the whole wave swept the culling table instead (the slow path). */
int trt_read_sweep_fallbacks(trt_context *ctx, unsigned long long *swept_traces);

/* Likewise: how many times a wave ran the shadow stage (over up to 64 hits each time).  hits / (64 * passes) is the lane
 * activity of the shadow stage; the hits of a frame are shadow_rays / number of lights. */
int trt_read_shading_passes(trt_context *ctx, unsigned long long *passes);

/* Likewise, the exact-test loops of the three kinds of trace (path rays TRT.c:1024, directional-light shadow rays TRT.c:907,
 * point-light shadow rays TRT.c:937): out[0..2] = wave-level iterations of each loop, out[3..5] = exact sphere tests summed over
 * lanes (tests / (64 * iterations) = the loop's lane activity: a wave iterates as long as its busiest lane), out[6] = point-light
 * shadow searches in which some lane's any-hit search was inconclusive and the wave ran the closest-hit search, out[7] = 0. */
int trt_read_loop_diagnostics(trt_context *ctx, unsigned long long out[8]);

/* Copy one light's table to the host (tests: the device-built table must equal the host reference builder's).
 * point_light: 0 = directional light `index`, 1 = point light `index`.  Returns the number of 64-bit words copied
 * (cells * ceil(N/64); cells = slabs * g^2 resp. shells * 6 g^2), 0 when the tables are off, or a negative TRT_ERR_*. */
long trt_read_light_grid(trt_context *ctx, int point_light, int index, unsigned long long *masks, size_t capacity_words);

/* Copy the LIST CELLS of one light's table -- the form the kernels read: one 64-bit cell per table cell (csrc/trt_raygrid.h),
 * packed on the device from the masks trt_read_light_grid returns -- and the scene's part of the pool of long lists, into which
 * the pooled cells' offsets point (tests: every cell must list the spheres of its mask, in ascending order).
 * point_light: 0 = directional light `index`, 1 = point light `index`.
 * info: {cells of the light's table, bits per list entry (8 or 16), pool words of the scene's part, 1 when the tables are on}.
 * cells = pool = NULL with both capacities 0 asks for the sizes only: info is filled and nothing is copied.
 * Returns the number of cells of the table, 0 when the tables are off, or a negative TRT_ERR_*. */
long trt_read_light_lists(trt_context *ctx, int point_light, int index, unsigned long long *cells, size_t capacity_cells,
                          unsigned long long *pool, size_t capacity_pool, long info[4]);

/* Device rounding self-test: quot[i] = a[i] / b[i], root[i] = sqrt(a[i]) computed by the same
 * device instructions sequences the kernels use (host arrays in/out). */
int trt_selftest_div_sqrt(trt_context *ctx, const double *a, const double *b, size_t n, double *quot, double *root);

/* The kernels normalise vectors (TRT.c:439-450) with one shared reciprocal refinement for the three divisions and a
 * square root without the compiler's range handling whenever a whole wave's operands are far from the ends of the
 * exponent range.  This entry runs that code (`fast`) and the compiler's plain `/` and sqrt (`reference`) on n
 * records {x, y, z, w}: out = {unit(x,y,z), sqrt(w)}.  The two outputs must be identical bit for bit. */
int trt_selftest_unit(trt_context *ctx, const double *xyzw, size_t n, double *fast, double *reference);

/* The candidate tables over cube maps (point lights, ray families, surface patches) take face and face coordinates of a
 * direction from gfx9's v_cubeid / v_cubesc / v_cubetc / v_cubema; the host-side builders and checkers use a C restatement of the
 * four instructions (csrc/trt_lightgrid.h, trt_cube_lookup).  n directions {x, y, z} in, {face, sc, tc, 2 * major} per direction out:
 * as the device computes them and as the host restatement does.  The two must agree bit for bit. */
int trt_selftest_cube(trt_context *ctx, const float *xyz, size_t n, float *device_out, float *host_out);

/* Tests: the skybox look-up of the production kernel (get_skybox_color, TRT.c:700-789) takes the texel's index from an FP32
 * estimate of the texel coordinates whenever that provably truncates as the reference's FP64 value does, and from the FP64 form
 * otherwise (csrc/trt_device.hpp: sky_index_estimate).  For n unit directions (3 doubles each) and a cubemap of side dim:
 * exact[i] = face dim^2 + vi dim + ui by the FP64 form, estimate[i] = by the estimate, ambiguous[i] != 0 where the estimate
 * does not vouch for itself.  The claim under test: ambiguous[i] == 0  =>  estimate[i] == exact[i]. */
int trt_selftest_sky(trt_context *ctx, const double *dirs, size_t n, int dim, long long *exact, long long *estimate, int *ambiguous);

/* Single-ray probe for tests: closest hit of TRT.c:793 for n rays (host arrays): obj[n],
 * point[3n], normal[3n], material[5n] (colour, reflectivity, specularity); lit[3n] = colour after
 * the lighting of TRT.c:894 for hits. */
int trt_probe_rays(trt_context *ctx, const Ray *rays, size_t n, int *obj, double *point, double *normal,
                   double *material, double *lit);

/* The same probe through the PRODUCTION kernel's stages (csrc/trt_rounds.hpp: candidate tables, fall-back sweep, exact
 * tests, surface record, lighting), so that trace_ray (TRT.c:793), ray_intersects_sphere/plane (:638, :677),
 * get_skybox_color (:700) and apply_lighting (:894) are each checked on the code that ships.  families[i] = the kernel's
 * family code of ray i (trt_path_family_code: 0 eye, 1 mirror eye, 2 + s starts on sphere s, codes from 2 + N on: mirror image
 * of a patch of a sphere; negative or families == NULL: none, the ray's wave sweeps); a ray that is not a member of the
 * family named falls back by itself.
 * camera: its origin is the eye the tables of families 0 and 1 are built for. */
int trt_probe_rays_production(trt_context *ctx, const Camera *camera, const Ray *rays, const int *families, size_t n, int *obj,
                              double *point, double *normal, double *material, double *lit);

/* WHERE THE DEVICE LOOKS (tests/test_device_lookups.py).  The candidate tables are proven conservative on the host, for the cell the
 * host headers look up; the three entries below make the device report its own choice, so that the host's proofs can be run on it.
 * Host arrays in and out, the context's stream, nothing on the product path.
 *
 * trt_probe_path_lookups: one lane per ray runs the render kernels' own look-up of a path ray's list cell (csrc/trt_rounds.hpp: path_cell, or
 * path_cell_patches when the scene has patches) on the scene image as the render kernel stages it -- for one camera, or, n_cameras = 2 ..
 * TRT_BATCH_MAX, as a batch launch stages it, frame b's eye tables in eye slot b; frames[i] < n_cameras is the frame of ray i (NULL: 0).
 * families[i]: the ray's family code as in trt_probe_rays_production (a code the kernel cannot decode counts as none).  Per ray:
 *   fallback   1: the ray's wave would sweep (no family, not a member of the family's table, or a cell without a list)
 *   cell_word  the list cell that was read, 0 if none was
 *   successor  with patches: the code path_cell_patches leaves for the ray's reflection by the ground; without: the code as it was looked up
 *   read_at    the index into the path rays' list cells that was read, -1: nothing was read (the ray failed the membership test)
 *   place      {region, table, cell} of read_at, split by the address ranges of the context's tables alone: region 0 the eye's tables (table =
 *              2 slot + family), 1 the 2 N P tables of the spheres (patch k of sphere i at i P + k, then the mirror images), 2 the lean twins
 *              (N P), -1 nothing read, -2 an index outside every table */
int trt_probe_path_lookups(trt_context *ctx, const Camera *cameras, int n_cameras, const Ray *rays, const int *families, const int *frames, size_t n,
                           int *fallback, unsigned long long *cell_word, int *successor, long long *read_at, int *place);

/* The look-up lines of the shading stage (csrc/trt_rounds.hpp: shadow_stage) for ONE light, in the kernel's light order (the directional
 * lights, then the point lights), on the headers the render kernel stages: per origin (3 doubles) far != 0 (the origin is not looked up),
 * the cell index trt_dirgrid_cell / trt_pointgrid_cell gives, the list cell read there (0 when far) and, for a point light, the bounds of
 * the any-hit search (trt_point_shadow_bounds of |light - o|^2 and of the unit direction's d.d; lo and hi may be NULL for a directional light). */
int trt_probe_shadow_lookups(trt_context *ctx, const double *origins, size_t n, int light, int *far, int *cell, unsigned long long *cell_word,
                             double *lo, double *hi);

/* trt_filter_setup on the device with the context's culling constants, then trt_filter_sign of every sphere of the staged culling table and,
 * if the scene has a directional light and sign_fixed != NULL, trt_filter_sign_fixed_dir with the staged row of directional light 0.
 * fields: the nine members of trt_ray_filter per ray as 32-bit words (the floats' bits, then ok); sign, sign_fixed: sphere-major,
 * [sphere * n + ray].  All IEEE operations: the host's must agree bit for bit. */
int trt_selftest_filter(trt_context *ctx, const Ray *rays, size_t n, unsigned *fields, unsigned *sign, unsigned *sign_fixed);

/* Measurement: the number of frames a context has launched so far (launch numbers count from 0), and the DEVICE time in ms from the
 * start of launch `first_launch` of context `first` to the end -- render kernel and ordered mean -- of launch `last_launch` of
 * context `last` (HIP events on the contexts' streams; both of one device; each among the last 256 launches of its context).
 * A pipelined loop deals its frames over several contexts: span / frames is its device time per frame, which bench.py prints
 * beside the host-clocked ms_per_step. */
long trt_launch_count(trt_context *ctx);
int trt_launch_span_ms(trt_context *first, long first_launch, trt_context *last, long last_launch, float *ms);

/* Where the production kernel and the reference-order kernel (trt_set_kernel(1)) read the scene from.  Every workgroup stages
 * an image of the scene (spheres, materials, lights, culling tables, table headers, camera, jitter) into LDS while it fits the
 * device's LDS; a scene whose image does not fit is read from an image in device memory instead, written per launch in the same
 * layout by one workgroup in front of the render kernel.  mode -1 (the default): device memory only when the LDS image of the
 * frame does not fit; 0: LDS only -- a scene that does not fit fails with TRT_ERR_CAPACITY, in trt_set_scene or, when only the
 * rays per pixel push it over, at render time; 1: device memory always (the same frames: for tests and A/B measurements).
 * The refraction extension has no device-memory form: such a scene fails at render time whatever the mode. */
int trt_set_scene_image(trt_context *ctx, int mode);

/* The scene image of the kernel trt_render_variant describes: in_device_memory 1 when it reads the image from device memory,
 * image_bytes its size (the production kernel's image for that launch's rays per pixel, or the reference-order kernel's records). */
int trt_render_image(trt_context *ctx, int *in_device_memory, unsigned long long *image_bytes);

/* TEST HOOK: make stale data visible.  Nothing clears the per-context sample scratch the production kernel writes (and the ordered
 * mean reads) or the framebuffer between launches: a render that drops a work unit finds the sample an earlier render of the same
 * frame left there, and the frame still comes out right.  on = 1: every launch first fills exactly its own sample range of the
 * scratch (pixels * rays per pixel * frames * 3 doubles) and exactly its own output range (pixels * frames * 3 doubles) with 0xFF
 * bytes -- a NaN in every double -- on the launch's stream; the reference-order kernel, which has no scratch, its output range.
 * A unit or a pixel that is not written then shows as NaN.  on = 0 (the default): a launch issues exactly what it issued before
 * there was this switch. */
int trt_set_scratch_fill(trt_context *ctx, int on);

/* TEST HOOK: allow (1) or forbid (0, the default) the environment variable TRT_RCCL_LIB to name the library that trt_dist_* binds in
 * RCCL's place (tests/rccl_stub.cpp: send / recv through shared memory, so that several ranks can share the one GPU of a test
 * box).  Must be called before the process's first use of RCCL: fails with TRT_ERR_NOT_INITIALISED once RCCL has been bound.  A
 * process that never calls it ignores the variable.  trt_dist_rccl_library() (trt_hip.h) says what was bound. */
int trt_dist_allow_rccl_override(int allow);

/* Tests of the drop-in layer (trt_hip.h section 1), which hands out no context: the default context behind project_scene and its
 * siblings, BORROWED -- NULL before the first call that creates it and after trt_shutdown, never to be destroyed by the caller, and
 * dangling once trt_shutdown or a trt_init of another device has destroyed it.  The getters of both headers may be called on it
 * between two drop-in calls of the same thread (trt_get_path_patches, trt_scene_info, trt_build_counts); nothing locks them. */
trt_context *trt_default_context(void);

/* What a context has built since it was created, two counts that only grow: table_builds, the builds of the scene's candidate
 * tables (light tables and sphere families together: one per trt_set_scene, per table setter with a scene in place, and per drop-in
 * call whose primitives changed or whose scene was promoted from moving to still), and skybox_uploads, the cubemaps sent to the
 * device.  The eye's two tables, rebuilt on the GPU per camera, are not counted.  Either pointer may be NULL. */
int trt_build_counts(trt_context *ctx, unsigned long long *table_builds, unsigned long long *skybox_uploads);

/* Measurement: trt_ansi_delta_from_rgb8_device (trt_hip.h) with a HIP event between its three kernels, SYNCHRONOUS: ms[0] the measure
 * kernel (record lengths, a sum per tile), ms[1] the offsets kernel (one workgroup's scan of the sums, the length), ms[2] the write
 * kernel (the records).  Same arguments, same text, same errors (tools/ansi_delta_bench.py). */
int trt_ansi_delta_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
/* The same of trt_ansi_delta_half_from_rgb8_device: its measure kernel, the shared offsets kernel, its write kernel
 * (tools/ansi_delta_half_bench.py). */
int trt_ansi_delta_half_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                     size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
/* The same of trt_ansi_delta_chain_from_rgb8_device and trt_ansi_delta_half_chain_from_rgb8_device: ms[0] the measure kernel over the
 * tiles of all n pairs of frames, ms[1] the one workgroup's scan of all their sums and the n lengths, ms[2] the write kernel.  Same
 * arguments, same texts, same errors (tools/ansi_delta_batch_bench.py). */
int trt_ansi_delta_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                      void *d_text, size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
int trt_ansi_delta_half_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                           void *d_text, size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
/* The four above of the delta texts in the xterm 256-colour palette (trt_ansi256_delta_from_rgb8_device and its _half and _chain forms):
 * the kind's measure kernel, the shared offsets kernel, the kind's write kernel (tools/ansi256_delta_bench.py). */
int trt_ansi256_delta_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                   size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
int trt_ansi256_delta_half_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows, void *d_text,
                                        size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
int trt_ansi256_delta_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                         void *d_text, size_t capacity_bytes, unsigned long long *d_bytes, float *ms);
int trt_ansi256_delta_half_chain_kernel_times(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                              void *d_text, size_t capacity_bytes, unsigned long long *d_bytes, float *ms);

#ifdef __cplusplus
}
#endif
#endif
