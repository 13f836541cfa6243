// trt_rounds.hpp -- production frame-producer kernel for gfx950: persistent waves, MODE-SYNCHRONOUS ROUNDS.
//
// Shape of the work: per pixel `spp` samples, per sample a bounce loop, per bounce one
// closest-hit trace plus one shadow trace per light; a trace = N sphere tests + 1 plane test.
//
// Work units are single SAMPLES (unit = pixel*spp + k), pulled from a global queue a chunk at a time into a
// wave-level pool.  A lane always owns exactly one pending PATH ray.  One round of the main loop advances
// every lane's path by one ray:
//
//   P      closest hit of the path ray, all lanes (TRT.c:1024)
//          sky  -> skybox texel, the sample ends (TRT.c:858-867, 1044-1048)
//          hit  -> nudged point, unit normal, material (TRT.c:868-886)
//   S(i)   for every light i (wave-uniform loop): shadow ray from the hit point for the lanes that hit something
//          (TRT.c:900-957); directional lights only ask "anything in the way?", so their search stops at the
//          first hit; lit colour accumulates in the reference's light order
//   END    bounce bookkeeping (TRT.c:1034-1056); a finished sample is normalised by its weight (TRT.c:1061),
//          written to f.samples[unit] and the lane pulls its next unit; one shared unit() gives every lane its
//          next direction (mirror reflection or fresh primary ray)
//
// Because all lanes of a wave are in the same stage, there is no per-lane state machine and no merging of
// modes; the code of each stage is straight-line with exec masking only for "hit" vs "sky".  The price is
// that lanes whose path ray reached the sky idle through the shadow stages of that round.
//
// The trace itself is a two-phase search.  Phase 1 proposes candidate spheres with ONE table look-up per ray: path rays
// come in families that (nearly) pass through one point -- the eye, its mirror image in the ground, a sphere, a sphere's
// mirror image -- and each family has a cube map of direction cells (trt_raygrid.h); the shadow rays of one light are a
// two-parameter family too (trt_lightgrid.h).  A cell is one 64-bit word holding up to seven sphere indices (longer lists
// live in a pool).  A ray that does not pass its family's membership test, or whose origin is outside a light table's
// range, makes its wave fall back to the wave-uniform FP32 sweep over a culling table in LDS (trt_filter.h: broadcast
// ds_read_b128, 9 VALU per sphere, verdict in a sign bit).  Phase 2 is per lane: the EXACT FP64 test of the few candidates
// in ascending index order.  No table or filter ever decides a hit.  FP64, contraction off: results are bit-identical to the
// reference.  The mean over a pixel's samples is formed by reduce_samples_kernel in the reference's order (TRT.c:1063-1065).
#pragma once

#include "trt_device.hpp"
#include "trt_filter.h"
#include "trt_lightgrid.h"
#include "trt_raygrid.h"
#include "trt_common.hpp"

// the whole-wave sweep and the closest-hit search of a point light are the rare ways: laid out as such (profiles/r05/f_ab_log.txt)
#define TRT_EXPECT_LIST(c) __builtin_expect(!!(c), 1)
#define TRT_EXPECT_RARE(c) __builtin_expect(!!(c), 0)

namespace trt
{


#define CONSTANT_AS __attribute__((address_space(4)))
// whole 64-bit words through the constant address space: scalar loads (the kernel's arguments; wave-uniform records)
template <class T>
TRT_DEV T load_kernel_argument(const char CONSTANT_AS *at)
{
    static_assert(sizeof(T) % 8 == 0 && alignof(T) == 8, "argument structs are whole 64-bit words");
    T out;
    const unsigned long long CONSTANT_AS *src = (const unsigned long long CONSTANT_AS *)at;
    unsigned long long *dst = (unsigned long long *)&out;
#pragma unroll
    for (size_t i = 0; i < sizeof(T) / 8; i++)
        dst[i] = src[i];
    return out;
}

// Candidate tables.  Every table cell is one 64-bit LIST CELL (trt_raygrid.h): up to seven sphere indices inline, longer
// lists in `pool`.
struct GridView
{
    // light-space tables of the shadow rays (trt_lightgrid.h): headers and one list cell per table cell
    const trt_dirgrid *dir;     // [num_dir]
    const trt_pointgrid *point; // [num_point]
    const unsigned long long *dir_lists, *point_lists;
    unsigned dir_stride, point_stride; // cells per light
    int enabled;
    int list_bits; // bits per entry of every list cell: 8, or 16 for scenes of more than 256 spheres (light tables only)
    // direction tables of the path rays' families (trt_raygrid.h): families 0 (eye) and 1 (mirror eye) have 6*g_eye^2 cells
    // each, from cell eye_at of path_lists (they change with the camera), then 2NP families (patch k of sphere i at i P + k, then
    // their mirror images) of 6*g_sph^2 cells, from cell sph_at (they change with the scene only)
    int path_enabled;
    int g_eye, g_sph;
    int patch_m, patch_count; // cells per face side of the origin's cube map (0: one family per sphere), P
    unsigned eye_at, sph_at;
    unsigned lean_off; // LEAN TWINS of the n P non-mirrored tables (trt_raygrid.h), in the same order, from cell sph_at + lean_off; 0: there are
                       // none, or they are switched off (an offset, not a second base: a select between two kernel arguments is a load from a
                       // private copy of them all)
    const unsigned long long *path_lists;
    const unsigned long long *pool;
    const double *sphere_fam; // per sphere: mirror image of the centre (3), then r_chk of the sphere's family (patch_m == 0) or |r|
    const double *patch_rec;  // per patch: t (3), rho | mirrored t (3), rho (TRT_PATCH_RECORD doubles)
    double rg2_sph;           // admissible |o - apex|^2 of the families of the spheres
    double slack0;            // membership radius of a patch's family = |r| rho + slack0 (TRT_FAMILY_SLACK more for its mirror image)
    trt_rayfamily eye[2];     // families 0 and 1, by value: they change with the camera
};

static_assert(sizeof(trt_rayfamily) == 8 * TRT_RAYFAMILY_DOUBLES, "families of the eye in the LDS image");
static_assert(sizeof(trt_dirgrid) == 8 * kDirGridDoubles && sizeof(trt_pointgrid) == 8 * kPointGridDoubles, "light-table headers in the LDS image");

constexpr int kDirRecord = 8; // doubles per directional light in the LDS image

struct LdsImage
{
    const float4 *cull;  // culling table {Cx,Cy,Cz,kk}
    const float4 *cull_dir; // per directional light: {Cx,Cy,Cz,kk - (C.d)^2}, `padded` entries each
    const double *sph;   // per sphere {cx, cy, cz, r^2}: one 32-byte record, 16-byte aligned, read with two ds_read_b128 by the exact
                         // test (measured 1.9 % faster than four ds_read_b64 from a structure of arrays)
    const double *mat;   // (n+2) x {colour, reflectivity, specularity}: spheres, ground even, ground odd
    const double *dir;   // per directional light (kDirRecord doubles): unit to-light (3), colour (3), then what every shadow ray towards it shares:
                         // a = d.d (TRT.c:643) and d.n of the ground test (TRT.c:679), formed once per workgroup from the same operands
    const double *pt;    // per point light: position (3), colour (3), intensity
    const double *b255;  // byte / 255.0
    const double *cam;   // basis x,y,z (9), eye (3), -screen_distance
    const double *jit;   // jitter x[spp], y[spp]
    const trt_dirgrid *dirgrid;     // headers of the light-space tables (trt_lightgrid.h), per directional light
    const trt_pointgrid *pointgrid; // per point light
    const double *fam;              // per sphere: mirror image of the centre (3), r_chk of its family or, with patches, |r| (trt_raygrid.h)
    const double *eye;              // the two families of the eye: 2 x {apex (3), r_chk, r_chk^2, rg^2}
    const double *patch;            // per patch of a sphere's surface: t (3), rho | mirrored t (3), rho
};

// LDS image of a workgroup: culling table {Cx,Cy,Cz,kk} (4 floats per sphere, 16-B aligned, first) | per sphere {cx,cy,cz,r^2} |
// mat[(n+2)*5] (spheres, ground even, ground odd) | dir lights: unit to-light(3) colour(3) | point lights: pos(3) colour(3)
// intensity | byte/255.0 [256] | camera | jitter x[spp] y[spp] | one fixed-direction culling table per directional
// light | headers of the light-space tables | per sphere {mirror centre, |r|} of the path-ray families | the two families
// of the eye | the patches of a sphere's surface (`patches` records).  rounds_lds_bytes and image_layout must agree: the layout
// ends at most rounds_lds_bytes from its base (the alignment double of the formula is always counted).
// `frames` > 1 (the BATCH instantiations, several cameras per launch): a camera block and a pair of eye families per frame, where
// a single frame has one of each; frames = 1 is the single-frame layout byte for byte.
inline size_t rounds_lds_bytes(const SceneView &s, int spp, int patches, int frames = 1)
{
    const size_t padded = ((size_t)s.num_spheres + kCullGroup - 1) / kCullGroup * kCullGroup;
    return sizeof(double) * (padded * 2 + (size_t)s.num_spheres * 4 + ((size_t)s.num_spheres + 2) * 5 + (size_t)s.num_dir * kDirRecord +
                             (size_t)s.num_point * 7 + 256 + kLdsCameraDoubles + 2 * (size_t)spp + 1 /* 16-B alignment */ +
                             (size_t)s.num_dir * padded * 2 + (size_t)s.num_dir * kDirGridDoubles + (size_t)s.num_point * kPointGridDoubles +
                             (size_t)s.num_spheres * 4 + 2 * TRT_RAYFAMILY_DOUBLES + (size_t)patches * TRT_PATCH_RECORD +
                             (size_t)(frames - 1) * (kLdsCameraDoubles + 2 * TRT_RAYFAMILY_DOUBLES));
}

// Where every part of the image lies from its base: one layout for the LDS image of a workgroup and for the device-memory image
// of a launch (render_rounds_kernel<.., DEVICE_IMAGE>, whose scene does not fit LDS).  The base must be 16-byte aligned.
struct ImageParts
{
    float4 *cull, *cull_dir;
    double *sph, *mat, *dir, *pt, *b255, *cam, *jit, *dirgrid, *pointgrid, *fam, *eye, *patch;
};

TRT_DEV ImageParts image_layout(double *base, int n, int nd, int np, int padded, int spp, int frames = 1)
{
    ImageParts p;
    p.cull = (float4 *)base;
    p.sph = base + padded * 2; // 16-byte aligned: the culling table before it is whole float4s
    p.mat = p.sph + 4 * n;
    p.dir = p.mat + (n + 2) * 5;
    p.pt = p.dir + nd * kDirRecord;
    p.b255 = p.pt + np * 7;
    p.cam = p.b255 + 256;
    p.jit = p.cam + frames * kLdsCameraDoubles;
    // fixed-direction tables behind everything else, on a 16-byte boundary (all offsets above are whole doubles)
    p.cull_dir = (float4 *)(base + (((p.jit + 2 * spp) - base + 1) & ~1L));
    // headers of the light-space tables behind the fixed-direction tables (whole doubles again: 4 floats per entry)
    p.dirgrid = (double *)(p.cull_dir + nd * padded);
    p.pointgrid = p.dirgrid + nd * kDirGridDoubles;
    p.fam = p.pointgrid + np * kPointGridDoubles;
    p.eye = p.fam + 4 * n;
    p.patch = p.eye + frames * 2 * TRT_RAYFAMILY_DOUBLES;
    return p;
}

TRT_DEV LdsImage image_view(const ImageParts &p)
{
    return LdsImage{p.cull, p.cull_dir, p.sph, p.mat, p.dir, p.pt, p.b255, p.cam, p.jit,
                    (const trt_dirgrid *)p.dirgrid, (const trt_pointgrid *)p.pointgrid, p.fam, p.eye, p.patch};
}

// The image of a frame, written by the threads of ONE workgroup (barriers between its phases): into LDS by every workgroup of the
// production kernel, or into device memory by stage_image_kernel (trt_render.hip) in front of a launch that reads it from there.
TRT_DEV void fill_image(const ImageParts &p, const SceneView &s, const CullView &cull, const FrameView &f, const GridView &grids)
{
    const int n = s.num_spheres, nd = s.num_dir, np = s.num_point;
    for (int i = threadIdx.x; i < cull.padded; i += blockDim.x)
        p.cull[i] = ((const float4 *)cull.table)[i];
    for (int i = threadIdx.x; i < n; i += blockDim.x)
    {
        const double *sp = s.spheres + (long)i * kSphereDoubles;
        p.sph[4 * i + 0] = sp[0];
        p.sph[4 * i + 1] = sp[1];
        p.sph[4 * i + 2] = sp[2];
        p.sph[4 * i + 3] = sp[3] * sp[3]; // radius*radius exactly as TRT.c:648 forms it
        for (int j = 0; j < 5; j++)
            p.mat[i * 5 + j] = sp[4 + j];
    }
    for (int i = threadIdx.x; i < 10; i += blockDim.x)
        p.mat[n * 5 + i] = s.ground[6 + i];
    for (int i = threadIdx.x; i < nd; i += blockDim.x)
    {
        const double *li = s.dir_lights + i * kDirLightDoubles;
        const d3 tl = unit(scale(load3(li), -1.0)); // TRT.c:903-904, the same value for every hit point
        p.dir[i * kDirRecord + 0] = tl.x, p.dir[i * kDirRecord + 1] = tl.y, p.dir[i * kDirRecord + 2] = tl.z;
        p.dir[i * kDirRecord + 3] = li[3], p.dir[i * kDirRecord + 4] = li[4], p.dir[i * kDirRecord + 5] = li[5];
        p.dir[i * kDirRecord + 6] = dot(tl, tl);                     // a of ray_intersects_sphere (TRT.c:643) for every shadow ray towards this light
        p.dir[i * kDirRecord + 7] = dot(tl, load3(s.ground + 3)); // d.n of ray_intersects_plane (TRT.c:679)
    }
    for (int i = threadIdx.x; i < np * 7; i += blockDim.x)
        p.pt[i] = s.point_lights[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        p.b255[i] = (double)i / 255.0; // TRT.c:866
    for (int i = threadIdx.x; i < 12; i += blockDim.x)
        p.cam[i] = f.cam[i];
    if (threadIdx.x < 3) // TRT.c:989, :1000-1002: basis z scaled by sz = -screen_distance, the same product for every primary ray
        p.cam[13 + threadIdx.x] = f.cam[6 + threadIdx.x] * -f.cam[12];
    if (threadIdx.x == 0)
        p.cam[12] = -f.cam[12];
    for (int i = threadIdx.x; i < 2 * f.spp; i += blockDim.x)
        p.jit[i] = f.jitter[i];
    __syncthreads();
    for (int i = threadIdx.x; i < nd * cull.padded; i += blockDim.x)
    {
        const int li = i / cull.padded, j = i - li * cull.padded;
        const float4 e = p.cull[j];
        const float dx = (float)p.dir[li * kDirRecord + 0], dy = (float)p.dir[li * kDirRecord + 1], dz = (float)p.dir[li * kDirRecord + 2]; // = trt_filter_setup's d
        p.cull_dir[i] = float4{e.x, e.y, e.z, trt_filter_fixed_dir_kk(e.x, e.y, e.z, e.w, dx, dy, dz)};
    }
    if (grids.enabled)
    {
        for (int i = threadIdx.x; i < nd * kDirGridDoubles; i += blockDim.x)
            p.dirgrid[i] = ((const double *)grids.dir)[i];
        for (int i = threadIdx.x; i < np * kPointGridDoubles; i += blockDim.x)
            p.pointgrid[i] = ((const double *)grids.point)[i];
    }
    if (grids.path_enabled)
    {
        for (int i = threadIdx.x; i < n * 4; i += blockDim.x)
            p.fam[i] = grids.sphere_fam[i];
        for (int i = threadIdx.x; i < 2 * TRT_RAYFAMILY_DOUBLES; i += blockDim.x)
            p.eye[i] = ((const double *)grids.eye)[i];
        for (int i = threadIdx.x; i < grids.patch_count * TRT_PATCH_RECORD; i += blockDim.x)
            p.patch[i] = grids.patch_rec[i];
    }
    __syncthreads();
    // A directional light's table is for rays along its UNIT direction (trt_lightgrid.h): a light whose direction could not be
    // normalised (TRT.c:444 leaves vectors shorter than 1e-4 alone) gets a range no origin is in -- "far" for every ray, its waves
    // sweep -- here, once per image, instead of the shading stage testing |sd.sd - 1| for every light in every pass.
    if (grids.enabled)
    {
        for (int i = threadIdx.x; i < nd; i += blockDim.x)
        {
            const d3 sd = load3(p.dir + i * kDirRecord);
            if (!(__builtin_fabs(dot(sd, sd) - 1.0) <= 9.094947017729282e-13))
                ((trt_dirgrid *)p.dirgrid)[i].rg2 = -1.0f;
        }
        __syncthreads();
    }
}

TRT_DEV LdsImage stage_lds_image(double *lds, const SceneView &s, const CullView &cull, const FrameView &f, const GridView &grids)
{
    const ImageParts p = image_layout(lds, s.num_spheres, s.num_dir, s.num_point, cull.padded, f.spp);
    fill_image(p, s, cull, f, grids);
    return image_view(p);
}

struct Hit
{
    double d2; // squared distance origin -> (un-nudged) hit point, TRT.c:815
    d3 p;      // hit point as the intersection routine produced it
    int i;     // -1: nothing; [0,n): sphere; n: ground
    double t;  // while the spheres are searched: the ray parameter of the best hit.  Its hit point p = o + t d (TRT.c:664-666) is
               // formed once, after the loop -- the same expression on the same operands: the same bits -- so that an iteration
               // replaces five registers with selects, not nine (round 3 measured this form no faster; on round 4's kernel, whose
               // VALU is the bound, it is: C5 +2.6 %)
};


// One EXACT sphere test of TRT.c:638-672 in the reference's operation order, folded into the running closest hit of
// TRT.c:808-826 (strict '<': the first index wins ties).  Predicated rather than branched: a lane without a candidate
// (`valid` false) tests sphere 0 and discards the result.  Returns true when an ANY_HIT search is answered.
// `inside` (refraction extension only, -1 otherwise): the sphere the ray travels inside of is met at the FAR root.
// UNIT_A (the candidates come from a table: every ray that is looked up has |a - 1| <= 2^-40): an ANY_HIT search does not form
// t0 = q / (2a), q = -b - sqrt(disc), at all -- t0 > 0 (TRT.c:659) holds iff q > 0 unless the quotient underflows, which a
// q > 2^-500 cannot; a q in (0, 2^-500] is divided as the reference divides it.
template <bool ANY_HIT, bool REFRACT = false, bool UNIT_A = false>
TRT_DEV bool exact_step(const LdsImage &L, d3 o, d3 d, double a, int i, bool valid, Hit &best, int inside = -1)
{
    static_assert(!(ANY_HIT && REFRACT), "shadow rays are the reference's");
    const double2 c01 = ((const double2 *)L.sph)[2 * i], c23 = ((const double2 *)L.sph)[2 * i + 1];
    const d3 c = d3{c01.x, c01.y, c23.x};
    const d3 oc = sub(o, c);
    const double b = 2.0 * dot(oc, d);
    const double cc = dot(oc, oc) - c23.y;
    const double disc = b * b - 4.0 * a * cc;
    const bool far_root = REFRACT && i == inside;
    bool done = false;
    if (valid && !(disc < 0.0) && (b < 0.0 || far_root)) // b >= 0  =>  -b - sqrt(disc) <= 0  =>  t0 <= 0 or NaN: a miss (TRT.c:657-659)
    { // no further branches: selects keep `best` in place (nested ifs cost five register copies per level)
        const double root = sqrt_exact(disc);
        if (ANY_HIT)
        { // "anything in the way?" (TRT.c:908): the first hit answers it; its position is never used
            const double q = -b - root;
            bool hit = UNIT_A ? q > TRT_SHADOW_QMIN : q / (2.0 * a) > 0.0;
            if (UNIT_A && q > 0.0 && !hit)
                hit = q / (2.0 * a) > 0.0;
            best.i = hit ? i : best.i;
            done = hit;
        }
        else
        {
            const double t0 = (far_root ? -b + root : -b - root) / (2.0 * a);
            const bool hit = t0 > 0.0;
            const d3 p = d3{o.x + t0 * d.x, o.y + t0 * d.y, o.z + t0 * d.z};
            const double d2 = dist2(o, p);
            const bool closer = hit && d2 < best.d2;
            best.d2 = closer ? d2 : best.d2;
            best.t = closer ? t0 : best.t;
            best.i = closer ? i : best.i;
        }
    }
    return done;
}

// Closest hit of TRT.c:793-856 for the lanes with `active`.  ANY_HIT: the caller only asks whether anything
// is hit (directional-light shadow ray, TRT.c:908), so a lane stops at its first hit and the ground is skipped
// once a sphere was found.
// `use_list` (wave-uniform): every active lane's candidates are the entries of its LIST CELL `cell` (trt_raygrid.h;
// indices ascending, up to seven inline, longer lists in `pool`).  Otherwise the wave sweeps the FP32 culling table
// (trt_filter.h) -- `fixed` != nullptr: all rays share the direction that culling table was built for -- and each lane
// pops its candidate bits.
// Lists longer than kListPrefilter entries in some lane of the wave are first thinned by the FP32 filter.
constexpr int kListPrefilter = 12;


template <bool ANY_HIT, bool REFRACT = false, int MARK_BASE = 0>
TRT_DEV Hit trace(const LdsImage &L, const CullView &cull, int n, d3 o, d3 d, bool active, unsigned long long active_lanes, d3 gp, d3 gn, unsigned &phase2_rounds, unsigned &lane_tests,
                  const float4 *fixed, bool use_list, unsigned long long cell, const unsigned long long *pool, int list_bits, int inside = -1,
                  const double *shared_ad = nullptr) // every lane's ray has the SAME direction (a directional light's shadow rays): {d.d, d.gn} from the LDS image
{
#define TRT_TRACE_MARK(k) TRT_MARK_AT(MARK_BASE + (k)) // MARK_BASE: the call site's slots (a template parameter: an immediate)
    (void)fixed;
    Hit best;
    best.d2 = __builtin_inf();
    best.p = o;
    best.i = -1;
    best.t = 0.0;
    const double a = shared_ad ? shared_ad[0] : dot(d, d);
    if (TRT_EXPECT_LIST(use_list))
    {
        const unsigned ctl = (unsigned)(cell >> 56);
        bool pooled = (ctl & TRT_LIST_POOLED) != 0;
        int count = active ? (pooled ? (int)((cell >> 32) & 0xffffu) : (int)ctl) : 0;
        const unsigned at = (unsigned)cell; // pooled: offset of the list's words
        const unsigned entry_mask = (1u << list_bits) - 1u;
        const int per_shift = list_bits == 8 ? 3 : 2, per_mask = (1 << per_shift) - 1; // 8 or 4 entries per pool word
        // The iterations that ask the lanes for a pool word are those with (k & per_mask) == fetch_at: 0 -- or, in a wave without a pooled list
        // (an inactive lane's cell is 0: not pooled), per_mask + 1, which no k meets: such a wave never takes the vote of the lanes.  A number in an
        // SGPR, not a condition (the empty asm): the loop's test stays one s_and and one s_cmp.
        int fetch_at = lanes_with(pooled) != 0 ? 0 : per_mask + 1;
        asm("" : "+s"(fetch_at));
        unsigned long long cur = cell;
        int k = 0;
        TRT_TRACE_MARK(0); // table load
        // Long lists (dense scenes): the FP32 filter of trt_filter.h first goes over the list -- 9 FP32 operations per entry
        // instead of ~19 FP64 -- and only the entries it cannot reject go to the exact test.  Like the sweep it never decides
        // a hit.  Up to eight survivors (four of 16 bits) fit one 64-bit word; if some lane has more, the wave tests its lists directly.
        if (__any(count > kListPrefilter))
        {
            trt_ray_filter flt;
            trt_filter_setup(&flt, o.x, o.y, o.z, d.x, d.y, d.z, a, cull.c0x, cull.c0y, cull.c0z, cull.cn, cull.rm);
            unsigned long long kept = 0, word = cell;
            int nk = 0;
            bool over = false;
            for (int j = 0; __any(j < count); j++)
            {
                const bool valid = j < count;
                if ((j & per_mask) == fetch_at) // the lanes are asked for a pool word only in the iterations that can need one
                    if (__any(valid && pooled))
                        if (valid && pooled)
                            word = pool[at + ((unsigned)j >> per_shift)];
                const unsigned i = valid ? (unsigned)word & entry_mask : 0u;
                word >>= list_bits;
                unsigned sign;
                if (ANY_HIT && fixed)
                {
                    const float4 e = fixed[i];
                    sign = trt_filter_sign_fixed_dir(&flt, e.x, e.y, e.z, e.w);
                }
                else
                {
                    const float4 e = L.cull[i];
                    sign = trt_filter_sign(&flt, e.x, e.y, e.z, e.w);
                }
                if (valid && (!flt.ok || !(sign >> 31)))
                {
                    over = over || nk > per_mask;
                    kept |= nk <= per_mask ? (unsigned long long)i << (list_bits * nk) : 0ull;
                    nk++;
                }
            }
            if (!__any(over))
            { // the survivors are the list now: ascending as before
                cur = kept;
                count = nk;
                pooled = false;
                fetch_at = per_mask + 1;
            }
        }
        TRT_TRACE_MARK(1);
        while (__any(k < count))
        {
            phase2_rounds++;
            const bool valid = k < count;
            lane_tests += valid;
            if ((k & per_mask) == fetch_at) // k is the wave's: seven iterations of eight ask nothing of the lanes
                if (__any(valid && pooled))
                    if (valid && pooled)
                        cur = pool[at + ((unsigned)k >> per_shift)];
            const int i = valid ? (int)((unsigned)cur & entry_mask) : 0;
            cur >>= list_bits;
            k++;
            if (exact_step<ANY_HIT, REFRACT, ANY_HIT>(L, o, d, a, i, valid, best, inside))
                count = 0;
        }
    }
    else
    {
        trt_ray_filter flt;
        trt_filter_setup(&flt, o.x, o.y, o.z, d.x, d.y, d.z, a, cull.c0x, cull.c0y, cull.c0z, cull.cn, cull.rm);
        TRT_TRACE_MARK(0);
        for (int base = 0; base < cull.padded; base += 64)
        {
            // phase 1: wave-uniform sweep; each verdict is a sign bit shifted into a per-lane word by v_alignbit,
            // sphere base+j ends up at bit 63-j of `cand`
            const int chunk = (cull.padded - base) < 64 ? (cull.padded - base) : 64;
            unsigned word[2];
#pragma unroll
            for (int h = 0; h < 2; h++)
            {
                const int first = base + 32 * h, count = (chunk - 32 * h) < 32 ? (chunk - 32 * h) : 32;
                unsigned bits = ~0u;
                for (int g = 0; g < count; g += kCullGroup)
                {
#pragma unroll
                    for (int j = 0; j < kCullGroup; j++)
                    {
                        if (ANY_HIT && fixed)
                        {
                            const float4 e = fixed[first + g + j];
                            bits = __builtin_amdgcn_alignbit(bits, trt_filter_sign_fixed_dir(&flt, e.x, e.y, e.z, e.w), 31);
                        }
                        else
                        {
                            const float4 e = L.cull[first + g + j]; // same address in every lane: LDS broadcast
                            bits = __builtin_amdgcn_alignbit(bits, trt_filter_sign(&flt, e.x, e.y, e.z, e.w), 31);
                        }
                    }
                }
                word[h] = count > 0 ? ~(bits << (32 - count)) & (count == 32 ? ~0u : ~((1u << (32 - count)) - 1u)) : 0u;
            }
            unsigned long long cand = ((unsigned long long)word[0] << 32) | word[1];
            if (!flt.ok)
                cand = chunk == 64 ? ~0ull : ~((1ull << (64 - chunk)) - 1ull); // degenerate ray: every sphere of the chunk
            if (!active)
                cand = 0;
            TRT_TRACE_MARK(1); // sweep
            // phase 2: exact FP64 tests of this lane's candidates, ascending index (first index wins ties, TRT.c:816)
            while (__any(cand != 0))
            {
                phase2_rounds++;
                const int lead = __builtin_clzll(cand | 1ull);
                const bool valid = cand != 0 && base + lead < n;
                lane_tests += valid;
                const int i = valid ? base + lead : 0;
                cand &= ~(0x8000000000000000ull >> lead);
                if (exact_step<ANY_HIT, REFRACT>(L, o, d, a, i, valid, best, inside))
                    cand = 0ull;
            }
        }
    }
    if (!ANY_HIT && best.i >= 0)
        best.p = d3{o.x + best.t * d.x, o.y + best.t * d.y, o.z + best.t * d.z}; // the winner's hit point: the expression of TRT.c:664-666 again
    TRT_TRACE_MARK(2); // exact tests
    // ground plane (TRT.c:831-853; ray_intersects_plane TRT.c:677-695).  One wave-level decision, then straight-line code with
    // selects: a ray can only hit if |d.n| > 1e-5 and numerator and denominator of t have the same sign (opposite signs: t <= 0,
    // whatever the quotient's digits are), so a wave whose rays all head away from the plane skips the division.
    {
        const double denom = shared_ad ? shared_ad[1] : dot(d, gn), num = dot(sub(gp, o), gn);
        const bool steep = __builtin_fabs(denom) > 0.00001;
        const bool same_sign = (long long)(__builtin_bit_cast(unsigned long long, num) ^ __builtin_bit_cast(unsigned long long, denom)) >= 0;
        const bool maybe = active && !(ANY_HIT && best.i >= 0) && steep && same_sign;
        unsigned long long maybe_lanes = active_lanes & lanes_with(steep) & lanes_with(same_sign);
        if (ANY_HIT)
            maybe_lanes &= ~lanes_with(best.i >= 0);
        if (maybe_lanes != 0)
        {
            const double t = num / denom;
            const bool hit = maybe && t > 0.00001;
            if (ANY_HIT)
                best.i = hit ? n : best.i; // nothing closer can matter: any hit blocks the light
            else
            {
                const d3 p = d3{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};
                const double d2 = dist2(o, p);
                const bool closer = hit && d2 < best.d2;
                best.d2 = closer ? d2 : best.d2;
                best.p.x = closer ? p.x : best.p.x;
                best.p.y = closer ? p.y : best.p.y;
                best.p.z = closer ? p.z : best.p.z;
                best.i = closer ? n : best.i;
            }
        }
    }
    TRT_TRACE_MARK(3); // plane
#undef TRT_TRACE_MARK
    return best;
}

// ANY-HIT search for the shadow ray of a POINT light (trt_lightgrid.h (4); TRT.c:937-942 asks for the closest blocker and whether
// it is nearer than the light): the candidates of the ray's list cell, then the ground.  `dark`: some hit is provably nearer than
// the light -- q > 2^-500 and q^2 (1 + 2^-30) <= lo, q = -b - sqrt(disc) the numerator of the near root (for the ground
// q = 2 a t) -- which decides the reference's answer whichever hit is the closest; the lane stops there.  A hit provably BEYOND
// the light (q^2 >= hi) cannot matter and is passed over.  `unsure`: the lane met a hit (q > 0) that is neither, and found no
// proof of "dark".  Neither flag: nothing nearer than the light is hit, the point is lit.  No division, no hit point, no running
// minimum: 3 FP64 operations and two compares per hit on top of the discriminant and its root.
TRT_DEV void point_light_search(const LdsImage &L, int n, d3 o, d3 d, bool active, unsigned long long active_lanes, d3 gp, d3 gn, unsigned &rounds, unsigned &lane_tests,
                                unsigned long long cell, const unsigned long long *pool, int list_bits, double lo, double hi, bool &dark, bool &unsure)
{
    (void)n;
    const double a = dot(d, d);
    const unsigned ctl = (unsigned)(cell >> 56);
    const bool pooled = (ctl & TRT_LIST_POOLED) != 0;
    int count = active ? (pooled ? (int)((cell >> 32) & 0xffffu) : (int)ctl) : 0;
    const unsigned at = (unsigned)cell;
    const unsigned entry_mask = (1u << list_bits) - 1u;
    const int per_shift = list_bits == 8 ? 3 : 2, per_mask = (1 << per_shift) - 1;
    int fetch_at = lanes_with(pooled) != 0 ? 0 : per_mask + 1; // as in trace(): a wave without a pooled list asks its lanes for no pool word
    asm("" : "+s"(fetch_at));
    unsigned long long cur = cell;
    int k = 0;
    dark = false, unsure = false;
    while (__any(k < count))
    {
        rounds++;
        const bool valid = k < count;
        lane_tests += valid;
        if ((k & per_mask) == fetch_at)
            if (__any(valid && pooled))
                if (valid && pooled)
                    cur = pool[at + ((unsigned)k >> per_shift)];
        const int i = valid ? (int)((unsigned)cur & entry_mask) : 0;
        cur >>= list_bits;
        k++;
        const double2 c01 = ((const double2 *)L.sph)[2 * i], c23 = ((const double2 *)L.sph)[2 * i + 1];
        const d3 oc = sub(o, d3{c01.x, c01.y, c23.x});
        const double b = 2.0 * dot(oc, d);
        const double cc = dot(oc, oc) - c23.y;
        const double disc = b * b - 4.0 * a * cc;
        if (valid && !(disc < 0.0) && b < 0.0) // b >= 0: t0 <= 0 or NaN, a miss (TRT.c:657-659)
        {
            const double q = -b - sqrt_exact(disc), qq = q * q;
            const bool blocks = q > TRT_SHADOW_QMIN && qq * TRT_SHADOW_K1 <= lo;
            unsure = unsure || (q > 0.0 && !blocks && !(qq >= hi));
            dark = dark || blocks;
            count = blocks ? 0 : count;
        }
    }
    // the ground (TRT.c:677-695) for the lanes that are not dark yet: one wave-level decision, as in trace() -- a ray can only
    // hit if |d.n| > 1e-5 and numerator and denominator of t have the same sign (opposite signs: t <= 0)
    {
        const double denom = dot(d, gn), num = dot(sub(gp, o), gn);
        const bool steep = __builtin_fabs(denom) > 0.00001;
        const bool same_sign = (long long)(__builtin_bit_cast(unsigned long long, num) ^ __builtin_bit_cast(unsigned long long, denom)) >= 0;
        // `dark` and `unsure` are set inside the loop's per-lane region: words of them would be per-lane values there (a merge behind
        // a divergent branch), so these two votes stay __any
        const bool maybe = active && !dark && steep && same_sign;
        if (__any(maybe))
        {
            const double t = num / denom;
            const bool hit = maybe && t > 0.00001;
            const double qq = (t * t) * (4.0 * a) * a; // q = 2 a t
            const bool blocks = hit && qq * TRT_SHADOW_K1 <= lo;
            dark = dark || blocks;
            unsure = unsure || (hit && !blocks && !(qq >= hi));
        }
    }
    unsure = unsure && !dark;
}

// The list cell of a PATH ray (trt_raygrid.h), ONE FAMILY PER SPHERE (GridView::patch_m == 0).  `fam`: the family the ray is
// expected in (0 eye, 1 mirror eye, 2 + i sphere i, 2 + n + i mirror sphere i, < 0 none).  `fallback_lanes` holds the active lanes
// whose ray fails the family's membership test (its line must pass within r_chk of the apex, its origin not more than r_chk
// behind it, within the table's range; a unit direction) or whose cell has no list: the caller then sweeps.  `active_lanes`:
// lanes_with(active) (trt_device.hpp).
// BATCH: the ray belongs to frame `frame` of a batch launch, whose eye families and tables it reads (0 and unused otherwise)
// DIAG (trt_probe_path_lookups only; the render kernels never set it): *read_at = the index into G.path_lists the lane read, -1: none
// `d_plain` (wave-uniform): `d` comes from unit_round() and the whole wave took its short way, so |d.d - 1| <= 2^-40 holds in every
// active lane (trt_device.hpp has the bound) and the membership's unit test is not run.  false: nothing is known, the test runs.
template <bool BATCH = false, bool DIAG = false>
TRT_DEV unsigned long long path_cell(const LdsImage &L, const GridView &G, int n, int fam, d3 o, d3 d, bool active, unsigned long long active_lanes,
                                     unsigned long long &fallback_lanes, int frame = 0, int inside = -1, long long *read_at = nullptr, bool d_plain = false)
{
    const bool in_family = fam >= 0;
    const unsigned long long family_lanes = lanes_with(in_family); // next to its compare: a vote on a compare of another block is a select and a compare again
    const bool has = active && in_family;
    const int f = has ? fam : 0;
    const int s = f >= 2 ? f - 2 : 0, i = s >= n ? s - n : s; // sphere of the family
    const bool of_eye = f < 2, mirrored = s >= n;
    const double *rec = L.fam + 4 * i; // mirror image of the centre, r_chk of the sphere's family
    d3 apex = mirrored ? load3(rec) : load3(L.sph + 4 * i);
    double r_chk = mirrored ? rec[3] + TRT_FAMILY_SLACK : rec[3];
    const double *E = BATCH ? L.eye + frame * (2 * TRT_RAYFAMILY_DOUBLES) + TRT_RAYFAMILY_DOUBLES * (f & 1) : L.eye + TRT_RAYFAMILY_DOUBLES * (f & 1);
    const double rg2_eye = E[5];
    if (of_eye)
    {
        apex = load3(E);
        r_chk = E[3];
    }
    const double rg2 = of_eye ? rg2_eye : G.rg2_sph; // by value: a pointer chosen between LDS and the kernel arguments is a flat load
    // trt_rayfamily_member, operation for operation (no branches between the first three conditions)
    const d3 w = sub(o, apex);
    const d3 c = d3{w.y * d.z - w.z * d.y, w.z * d.x - w.x * d.z, w.x * d.y - w.y * d.x};
    const double along = dot(w, d);
    const bool near_line = dot(c, c) <= r_chk * r_chk, ahead = along >= -r_chk, in_range = dot(w, w) <= rg2;
    bool member = near_line & ahead & in_range;
    unsigned long long member_lanes = family_lanes & lanes_with(near_line) & lanes_with(ahead) & lanes_with(in_range);
    if (TRT_EXPECT_RARE(!d_plain)) // the fourth condition, where unit_round() has not already settled it for the wave
    {
        const bool unit_dir = __builtin_fabs(dot(d, d) - 1.0) <= 9.094947017729282e-13;
        member &= unit_dir;
        member_lanes &= lanes_with(unit_dir);
    }
    const int g = of_eye ? G.g_eye : G.g_sph;
    const int at = trt_cubemap_cell((float)d.x, (float)d.y, (float)d.z, 0.5f * (float)g, (float)(g - 1), g);
    const unsigned eye_cells = 6u * (unsigned)G.g_eye * (unsigned)G.g_eye, sph_cells = 6u * (unsigned)G.g_sph * (unsigned)G.g_sph;
    // A ray of sphere i's own family that leaves the surface outwards reads the LEAN TWIN of its cell, the list without i
    // (trt_raygrid.h): `along` is then dot(sub(o, c_i), d) of the very operands exact_step reads -- the same LDS record -- so
    // b = 2 along there, and b >= 0 is that test's own "miss".  (The sphere a refracted ray travels inside of is met at the far
    // root whatever b is: such a ray keeps the full list.)  NaN, a negative dot, every other family: the full table.
    const bool outwards = f >= 2 && !mirrored && along >= 0.0 && i != inside;
    const unsigned base = of_eye ? G.eye_at + (BATCH ? 2u * (unsigned)frame + (unsigned)f : (unsigned)f) * eye_cells
                                 : G.sph_at + (outwards ? G.lean_off : 0u) + (unsigned)s * sph_cells;
    unsigned long long cell = 0;
    if (has && member)
        cell = G.path_lists[base + (unsigned)at];
    if constexpr (DIAG)
        *read_at = has && member ? (long long)(base + (unsigned)at) : -1;
    fallback_lanes = active_lanes & (~member_lanes | lanes_with((unsigned)(cell >> 56) == TRT_LIST_NONE)); // active && (!has || !member || no list)
    return cell;
}

// The same with the surface of every sphere cut into PATCHES that have a family each (GridView::patch_m > 0, trt_raygrid.h).
// `fam`: the family code of the ray (0 eye, 1 mirror eye, 2 + i: it starts on
// sphere i -- the patch of the sphere's surface follows from the origin --, 2 + n + (i << TRT_PATCH_SHIFT | k): reflected by the
// ground, its parent started on patch k of sphere i; < 0 none).  `fam` becomes the family code of the ray's REFLECTION BY THE
// GROUND, should it go on to hit the ground: the mirror family of this one's -- of the patch the ray started on -- or none (a ray
// from the ground cannot hit the ground again).  `fallback_lanes` holds the active lanes whose ray fails the family's
// membership test (its line must pass within r_chk of the apex, its origin not more than r_chk behind it, within the table's
// range; a unit direction) or whose cell has no list: the caller then sweeps.
// DIAG, `d_plain`: as in path_cell.
template <bool BATCH = false, bool DIAG = false>
TRT_DEV unsigned long long path_cell_patches(const LdsImage &L, const GridView &G, int n, int &fam, d3 o, d3 d, bool active, unsigned long long active_lanes,
                                             unsigned long long &fallback_lanes, int frame = 0, int inside = -1, long long *read_at = nullptr, bool d_plain = false)
{
    const bool in_family = fam >= 0;
    const unsigned long long family_lanes = lanes_with(in_family); // next to its compare: a vote on a compare of another block is a select and a compare again
    const bool has = active && in_family;
    const int f = has ? fam : 0;
    const bool of_eye = f < 2, mirrored = f >= 2 + n;
    const int code = f - 2 - n; // mirrored: sphere and patch
    const int i = mirrored ? code >> TRT_PATCH_SHIFT : (of_eye ? 0 : f - 2); // sphere of the family
    // ONE record read per lane, from wherever the family's base point lives (all of it is in LDS: the choice is a 32-bit
    // select of the address): the sphere's centre, its mirror image, or the eye / mirror eye, whose families are "patches" of
    // a sphere of radius 0 -- base + 0 t is the base, 0 rho + slack the slack
    const double *at_sphere = L.sph + 4 * i, *at_mirror = L.fam + 4 * i;
    const double *src = of_eye ? L.eye + (BATCH ? frame * (2 * TRT_RAYFAMILY_DOUBLES) : 0) + TRT_RAYFAMILY_DOUBLES * (f & 1) : (mirrored ? at_mirror : at_sphere);
    const d3 base_at = load3(src);
    // which patch of its sphere the ray starts on (FP32: the membership test below is what counts)
    const d3 from_base = sub(o, base_at);
    const int here = trt_cubemap_cell((float)from_base.x, (float)from_base.y, (float)from_base.z, 0.5f * (float)G.patch_m, (float)(G.patch_m - 1), G.patch_m);
    const int k = mirrored ? code & ((1 << TRT_PATCH_SHIFT) - 1) : (of_eye ? 0 : here);
    fam = !has ? -1 : (f == 0 ? 1 : (!of_eye && !mirrored ? 2 + n + (((f - 2) << TRT_PATCH_SHIFT) | k) : -1)); // a ray without a family has no successor family either
    const double r_abs = of_eye ? 0.0 : at_mirror[3];
    const double *pr = L.patch + TRT_PATCH_RECORD * k + (mirrored ? 4 : 0);
    const d3 apex = d3{TRT_PATCH_APEX(base_at.x, r_abs, pr[0]), TRT_PATCH_APEX(base_at.y, r_abs, pr[1]), TRT_PATCH_APEX(base_at.z, r_abs, pr[2])};
    const double rho = pr[3];
    // the eye's own radius and range come from LDS, the spheres' from the kernel's arguments.  Values first, selects after: a
    // select between a POINTER into LDS and one to the (re-read) arguments is a flat load from a private copy
    double rchk_eye = src[3], rg2_eye = src[5]; // only meaningful where src is a family of the eye
    asm("" : "+v"(rchk_eye), "+v"(rg2_eye));
    double r_chk = TRT_PATCH_RCHK(r_abs, rho, G.slack0), rg2 = G.rg2_sph;
    r_chk = mirrored ? r_chk + TRT_FAMILY_SLACK : r_chk;
    r_chk = of_eye ? rchk_eye : r_chk;
    rg2 = of_eye ? rg2_eye : rg2;
    // trt_rayfamily_member, operation for operation (no branches between the first three conditions)
    const d3 w = sub(o, apex);
    const d3 c = d3{w.y * d.z - w.z * d.y, w.z * d.x - w.x * d.z, w.x * d.y - w.y * d.x};
    const bool near_line = dot(c, c) <= r_chk * r_chk, ahead = dot(w, d) >= -r_chk, in_range = dot(w, w) <= rg2;
    bool member = near_line & ahead & in_range;
    unsigned long long member_lanes = family_lanes & lanes_with(near_line) & lanes_with(ahead) & lanes_with(in_range);
    if (TRT_EXPECT_RARE(!d_plain)) // the fourth condition, where unit_round() has not already settled it for the wave
    {
        const bool unit_dir = __builtin_fabs(dot(d, d) - 1.0) <= 9.094947017729282e-13;
        member &= unit_dir;
        member_lanes &= lanes_with(unit_dir);
    }
    const int g = of_eye ? G.g_eye : G.g_sph;
    const int at = trt_cubemap_cell((float)d.x, (float)d.y, (float)d.z, 0.5f * (float)g, (float)(g - 1), g);
    const unsigned eye_cells = 6u * (unsigned)G.g_eye * (unsigned)G.g_eye, sph_cells = 6u * (unsigned)G.g_sph * (unsigned)G.g_sph;
    const unsigned table = ((mirrored ? (unsigned)n : 0u) + (unsigned)i) * (unsigned)G.patch_count + (unsigned)k;
    // the LEAN TWIN for a ray that leaves its sphere outwards, as in path_cell: there the base point is the centre, from_base the
    // exact test's o - c_i from the same LDS record, and the dot half its b
    const bool outwards = !of_eye && !mirrored && dot(from_base, d) >= 0.0 && i != inside;
    const unsigned base = of_eye ? G.eye_at + (BATCH ? 2u * (unsigned)frame + (unsigned)f : (unsigned)f) * eye_cells
                                 : G.sph_at + (outwards ? G.lean_off : 0u) + table * sph_cells;
    unsigned long long cell = 0;
    if (has && member)
        cell = G.path_lists[base + (unsigned)at];
    if constexpr (DIAG)
        *read_at = has && member ? (long long)(base + (unsigned)at) : -1;
    fallback_lanes = active_lanes & (~member_lanes | lanes_with((unsigned)(cell >> 56) == TRT_LIST_NONE)); // active && (!has || !member || no list)
    return cell;
}

// how many lanes below this one are set in `mask` (v_mbcnt: no lane mask to keep in registers)
TRT_DEV unsigned lanes_below(unsigned long long mask)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// Per-lane counters of the counting kernel variant, handed through the stages.
struct Tally
{
    unsigned path = 0, shadow = 0, rounds = 0, swept = 0, passes = 0;
    unsigned iters[3] = {0, 0, 0}; // wave-level iterations of the exact-test loops: path rays, directional-light shadow rays, point-light ones
    unsigned tests[3] = {0, 0, 0}; // exact tests of THIS lane in those loops (tests / (64 iters) = the loops' lane activity)
    unsigned full = 0;             // point-light shadow searches that fell back from the any-hit form to the closest-hit one
};

// What the path ray of a round found (TRT.c:793-889).
struct PathHit
{
    Hit ph;     // closest hit as the intersection routine produced it (un-nudged point)
    bool hit;   // a sphere or the ground
    bool sky;   // nothing: the sample ends on the sky
    unsigned long long hit_lanes, sky_lanes; // lanes_with(hit), lanes_with(sky) (trt_device.hpp)
    d3 back;    // hit: unit vector back along the ray (nudge direction, TRT.c:871-872); sky: the unit direction (TRT.c:702, :878)
    d3 normal;  // hit: unit surface normal (TRT.c:878)
    int mat;    // hit: index into L.mat (sphere i, n = ground even, n + 1 = ground odd; TRT.c:850-851)
};

// P: closest hit of the path ray (o, d) of every lane with `alive`, candidates from the table of the ray's family `fam`
// (trt_raygrid.h) unless some lane's ray is not a member of its family; then the surface record.  `fam` becomes the family of
// the NEXT path ray: it starts on the sphere that was hit, or it is the mirror image in the ground of a ray of this one's
// family -- of the patch of its sphere this ray started on -- (a ray from the ground cannot hit the ground again; if it
// does, it has no family).
template <bool COUNT, bool REFRACT = false, bool PATCHES = false, bool BATCH = false>
TRT_DEV PathHit path_stage(const LdsImage &L, const CullView &cull, const GridView &grids, int n, d3 o, d3 d, int &fam, bool alive, unsigned long long alive_lanes,
                           d3 gp, d3 gn, Tally &tally, int inside = -1, int frame = 0, bool d_plain = false) // d_plain: see path_cell
{
    bool p_list = false;
    unsigned long long p_cell = 0;
    if (grids.path_enabled)
    {
        unsigned long long fallback_lanes;
        if constexpr (PATCHES)
            p_cell = path_cell_patches<BATCH>(L, grids, n, fam, o, d, alive, alive_lanes, fallback_lanes, frame, REFRACT ? inside : -1, nullptr, d_plain); // fam: now what a reflection by the ground belongs to
        else
            p_cell = path_cell<BATCH>(L, grids, n, fam, o, d, alive, alive_lanes, fallback_lanes, frame, REFRACT ? inside : -1, nullptr, d_plain);
        p_list = fallback_lanes == 0;
    }
    if (COUNT && !p_list)
        tally.swept++;
    PathHit r;
    r.ph = trace<false, REFRACT, 2>(L, cull, n, o, d, alive, alive_lanes, gp, gn, tally.iters[0], tally.tests[0], nullptr, p_list, p_cell, grids.pool, grids.list_bits, inside);
    r.hit = alive && r.ph.i >= 0;
    r.sky = alive && r.ph.i < 0;
    r.hit_lanes = alive_lanes & lanes_with(r.ph.i >= 0);
    r.sky_lanes = alive_lanes & ~r.hit_lanes;
    if (r.hit)
        fam = r.ph.i < n ? 2 + r.ph.i : (PATCHES ? fam : (fam == 0 ? 1 : (fam >= 2 && fam < 2 + n ? fam + n : -1)));
    // one unit() for "back along the ray" (nudge, TRT.c:871-872) or the sky direction (TRT.c:702), one for the normal
    r.back = unit_round(r.hit ? sub(o, r.ph.p) : d);
    r.normal = d;
    r.mat = 0;
    if (r.hit_lanes != 0)
    {
        d3 raw = gn;
        r.mat = n + checker_odd(r.ph.p); // TRT.c:850-851 (only meaningful for a ground hit)
        if (r.ph.i >= 0 && r.ph.i < n)
        {
            raw = sub(r.ph.p, load3(L.sph + 4 * r.ph.i)); // TRT.c:824
            r.mat = r.ph.i;
        }
        r.normal = unit_round(raw); // TRT.c:878
    }
    TRT_MARK_AT(6); // P post: nudge direction, normal
    return r;
}

// The exponent of the specular extension from a material's specularity e: 0 unless e >= 0 (negative values, NaN), 65535 from there
// up, otherwise e truncated.
TRT_DEV int specular_exponent(double e)
{
    return !(e >= 0.0) ? 0 : (e >= 65535.0 ? 65535 : (int)e);
}

// c^n by binary exponentiation, right to left, every product ONE rounded FP64 multiplication (no contraction: there is nothing to
// contract with), so that a CPU restatement and an exact model reach the same bits -- pow() is correctly rounded neither in glibc nor in
// the device library.  n = 0 gives 1.0, as pow(c, 0) does.  The lanes of a wave loop to the wave's largest n; a lane whose n is
// exhausted has left the loop's exec mask and multiplies nothing.  n = 100, the demo's, is six squarings and two products.
TRT_DEV double specular_power(double c, int n)
{
    double r = 1.0, b = c;
    while (n)
    {
        if (n & 1)
            r = r * b;
        n >>= 1;
        if (n)
            b = b * b;
    }
    return r;
}

// S(i): lighting of TRT.c:894-957 for the lanes with `lit_lanes`: one shadow ray per light from the (nudged) surface point
// `o` with unit normal `normal`, candidates from the light's table (trt_lightgrid.h) unless some lane's origin is outside
// its range; the lit colour is accumulated in the reference's light order, NOT yet clamped (TRT.c:960).
// SPECULAR (EXTENSION, parity unpinned; the declared rules are in include/trt_hip.h above trt_set_specular): every light that reaches
// the point also adds its Blinn-Phong term -- the lines the reference keeps commented out (TRT.c:913-916, :921, :947-950, :955) with
// specular_power in pow's place -- after its diffuse term and before the clamp.  `view`: minus the path ray's unit direction (TRT.c:1029).
template <bool COUNT, bool SPECULAR = false>
TRT_DEV d3 shadow_stage(const LdsImage &L, const CullView &cull, const GridView &grids, int n, int nd, int nl, d3 o, d3 normal, int mat,
                        bool lit_lanes, unsigned long long lit_word, d3 gp, d3 gn, Tally &tally, // lit_word: lanes_with(lit_lanes) (trt_device.hpp)
                        d3 view = d3{0.0, 0.0, 0.0})
{
    d3 lit = d3{0.0, 0.0, 0.0};
    if (lit_word == 0)
        return lit;
    int spec_n = 0; // the exponent of the hit material, formed once for all lights
    if constexpr (SPECULAR)
        spec_n = specular_exponent(L.mat[mat * 5 + 4]);
    for (int li = 0; li < nl; li++)
    {
        if (COUNT && lit_lanes)
            tally.shadow++;
        d3 sd, lcolor;
        bool is_lit;
        double factor;
        [[maybe_unused]] double spec_scale = 0.0; // SPECULAR, point lights: light_intensity
        if (li < nd)
        { // directional light, TRT.c:900-923
            TRT_MARK_AT(24); // ISA profile: a directional light's pass starts
            sd = load3(L.dir + li * kDirRecord);
            lcolor = load3(L.dir + li * kDirRecord + 3);
            bool use_list = false;
            unsigned long long cell = 0;
            if (grids.enabled)
            {
                const trt_dirgrid *G = L.dirgrid + li; // header in LDS: a global read here would sit in front of the cell's load
                int far;
                const int c = trt_dirgrid_cell(G, o.x, o.y, o.z, &far); // a light without a unit direction: far (stage_lds_image)
                if (lit_lanes && !far)
                    cell = grids.dir_lists[(size_t)li * grids.dir_stride + (unsigned)c];
                use_list = (lit_word & (lanes_with(far != 0) | lanes_with((unsigned)(cell >> 56) == TRT_LIST_NONE))) == 0;
            }
            if (COUNT && !use_list)
                tally.swept++;
            TRT_MARK_AT(8); // look-up
            const Hit sh = trace<true, false, 9>(L, cull, n, o, sd, lit_lanes, lit_word, gp, gn, tally.iters[1], tally.tests[1], L.cull_dir + li * cull.padded, use_list, cell, grids.pool, grids.list_bits,
                                                 -1, L.dir + li * kDirRecord + 6);
            is_lit = sh.i < 0;
            factor = min1(dot(normal, sd));
            TRT_MARK_AT(13); // directional shadow tail
        }
        else
        { // point light, TRT.c:926-957
            TRT_MARK_AT(25); // ISA profile: a point light's pass starts
            const double *pl = L.pt + (li - nd) * 7;
            const d3 to_light = sub(load3(pl), o);
            const double light_d2 = dot(to_light, to_light);
            const double strength = clampd(pl[6] / light_d2, 0.0, 1.0);
            bool sd_plain;
            sd = unit_round(to_light, sd_plain);
            lcolor = load3(pl + 3);
            bool use_list = false;
            unsigned long long cell = 0;
            if (grids.enabled)
            {
                const trt_pointgrid *G = L.pointgrid + (li - nd);
                int far;
                const int c = trt_pointgrid_cell(G, o.x, o.y, o.z, &far);
                if (TRT_EXPECT_RARE(!sd_plain)) // otherwise known to hold for the wave (unit_round, trt_device.hpp)
                    far |= !(__builtin_fabs(dot(sd, sd) - 1.0) <= 9.094947017729282e-13);
                if (lit_lanes && !far)
                    cell = grids.point_lists[(size_t)(li - nd) * grids.point_stride + (unsigned)c];
                use_list = (lit_word & (lanes_with(far != 0) | lanes_with((unsigned)(cell >> 56) == TRT_LIST_NONE))) == 0;
            }
            if (COUNT && !use_list)
                tally.swept++;
            TRT_MARK_AT(14); // unit(to_light), strength, look-up
            // ANY-HIT search (trt_lightgrid.h (4)): a candidate that is provably hit nearer than the light proves "dark", whichever
            // hit is the closest; no hit at all is "lit"; anything else (a blocker about as far as the light) leaves the lane
            // unsure and sends its wave through the closest-hit search of TRT.c:937-942 below.
            bool full = !use_list;
            is_lit = true;
            if (use_list)
            {
                const trt_pointgrid *G = L.pointgrid + (li - nd);
                double lo, hi;
                trt_point_shadow_bounds(G, light_d2, dot(sd, sd), &lo, &hi);
                bool dark, unsure;
                point_light_search(L, n, o, sd, lit_lanes, lit_word, gp, gn, tally.iters[2], tally.tests[2], cell, grids.pool, grids.list_bits, lo, hi, dark, unsure);
                is_lit = !dark;
                full = __any(lit_lanes && unsure);
                TRT_MARK_AT(17); // any-hit search
            }
            if (TRT_EXPECT_RARE(full))
            {
                if (COUNT)
                    tally.full++;
                const Hit sh = trace<false, false, 26>(L, cull, n, o, sd, lit_lanes, lit_word, gp, gn, tally.iters[2], tally.tests[2], nullptr, use_list, cell, grids.pool, grids.list_bits);
                is_lit = sh.i < 0;
                // A blocker: is it farther than the light?  The reference compares light_d2 with the squared distance to the
                // blocker point NUDGED 1e-6 back along the ray (TRT.c:871-874, :939-942): (D - 1e-6)^2 up to ~1e-14 relative
                // rounding, where D^2 = sh.d2 (1 +- 4u).  From D <= (D^2+1)/2:
                //     (D-1e-6)^2 (1-1e-14)  >=  sh.d2 (1 - 1.01e-6) - 1.01e-6      and, for D >= 1e-5,   (D-1e-6)^2 (1+1e-14) < sh.d2.
                // Outside that band the answer is certain without normalising anything; inside it the exact nudged point is
                // formed as the reference does.
                const bool surely_lit = light_d2 < sh.d2 * (1.0 - 1.01e-6) - 1.01e-6;
                const bool surely_dark = sh.d2 > 1e-10 && light_d2 >= sh.d2;
                if (sh.i >= 0)
                    is_lit = surely_lit;
                if (__any(lit_lanes && sh.i >= 0 && !surely_lit && !surely_dark))
                {
                    const d3 to_blocker = sub(add(sh.p, scale(unit(sub(o, sh.p)), 0.000001)), o);
                    if (sh.i >= 0 && !surely_lit && !surely_dark)
                        is_lit = light_d2 < dot(to_blocker, to_blocker);
                }
            }
            factor = strength * min1(dot(normal, sd));
            if constexpr (SPECULAR)
                spec_scale = strength;
            TRT_MARK_AT(19); // point shadow tail
        }
        if (lit_lanes && is_lit)
        {
            lit = add(lit, mulc(scale(lcolor, factor), load3(L.mat + mat * 5)));
            if constexpr (SPECULAR)
            { // TRT.c:914-916 / :948-950, then :921 / :955: not multiplied by the material's colour
                const d3 half = unit(add(sd, view));
                const double s = specular_power(clampd(dot(normal, half), 0.0, 1.0), spec_n);
                lit = add(lit, scale(lcolor, li < nd ? s : spec_scale * s)); // a point light: ONE product first, then the scale
            }
        }
    }
    return lit;
}

// Register budget: asking the allocator for only 3 waves/SIMD lets it settle at 127 VGPRs -- which still runs 4 waves/SIMD
// (<= 128) -- with a better schedule than when it is forced under 128 (measured 3.02 vs 3.15 ms).  The build records the
// compiler's resource report in build/resource_usage.txt and `make lib` warns if this kernel ever needs more than 128.
#ifndef TRT_ROUNDS_WAVES
#if TRT_BLOCK > 768
#define TRT_ROUNDS_WAVES 4 // a 1024-thread workgroup is 4 waves per SIMD by itself
#else
#define TRT_ROUNDS_WAVES 3
#endif
#endif

// REFRACT (EXTENSION, parity unpinned: the reference has no refraction): f.ior[i] > 0 makes sphere i a refractor.  A path
// ray that hits it from outside is shaded like any hit and continues along the refracted direction from a point 1e-6 PAST
// the surface; inside, that sphere is met at its far root; leaving it adds no colour and no weight but costs a bounce; total
// internal reflection mirrors the ray.  Restated operation for operation in oracle/trt_oracle.c (shade_pixel_refractive).
// The default instantiation (REFRACT = false) is the reference's path, unchanged.
//
// COMPACT: the shading of a hit (the shadow rays of S and the clamp, TRT.c:894-962) is decoupled from the lane that owns the
// sample.  A hit becomes a TASK {nudged point, normal, material, weight} in a ring in LDS that belongs to the wave; the wave
// shades tasks 64 at a time, whichever lanes they came from, and a task may wait for the NEXT round's hits to fill the pass
// it runs in -- never longer, so that a lane has at most two colours outstanding and they reach its sample in bounce order
// (TRT.c:1040 adds them in that order; the sky colour of TRT.c:1044 after them).  What is computed for a task is what the
// owner would have computed, operation for operation; only WHICH lane computes it, and when, changes.
constexpr int kRingTasks = 128;                            // >= 63 carried over + 64 new
constexpr int kRingDoubles = 7 * kRingTasks + kRingTasks / 4 + 3 * 64; // point(3) normal(3) weight(1) as arrays of doubles, material as 16-bit ints;
                                                                        // then per LANE the direction of its next path ray while the wave shades

// The kernel's arguments live in the kernarg segment (constant address space, read with scalar loads).  Held in SGPRs for the
// whole kernel they do not fit: the compiler spilt ~75 of them to VGPR lanes and read ~110 back per round with v_readlane, a
// tenth of the VALU instructions.  TRT_FRESH_ARGS re-reads, at the head of a stage, the arguments that stage uses (the copies
// shadow the kernel's parameters; unused fields are never loaded): a few s_load per stage instead of the v_readlanes, and
// nothing to keep alive between stages.  The empty asm makes the pointer opaque so that the loads stay where they are written.
constexpr size_t kArgScene = 0;
constexpr size_t kArgCull = (kArgScene + sizeof(SceneView) + alignof(CullView) - 1) / alignof(CullView) * alignof(CullView);
constexpr size_t kArgFrame = (kArgCull + sizeof(CullView) + alignof(FrameView) - 1) / alignof(FrameView) * alignof(FrameView);
constexpr size_t kArgGrids = (kArgFrame + sizeof(FrameView) + alignof(GridView) - 1) / alignof(GridView) * alignof(GridView);
// the explicit arguments of a kernel sit in the kernarg segment like the members of a struct, from offset 0
struct RenderKernelArguments
{
    SceneView s;
    CullView cull;
    FrameView f;
    GridView grids;
};
static_assert(offsetof(RenderKernelArguments, cull) == kArgCull && offsetof(RenderKernelArguments, f) == kArgFrame &&
                  offsetof(RenderKernelArguments, grids) == kArgGrids,
              "TRT_FRESH_ARGS reads the kernel's arguments at these offsets");

// BATCH (trt_render_device_batch): ONE launch works through the samples of up to kBatchMax frames of one scene.  The units are
// frame-major (unit = frame * units_per_frame + pixel * spp + k) in the one queue of the launch, so that the tail of frame b is
// filled by the head of frame b + 1.  What depends on the camera comes by value in a fifth kernel argument -- a batch still in
// flight never shares a buffer with the next one -- and is staged into the image: a camera block and a pair of eye families per
// frame.  Frame b's two eye tables are cells [eye_at + 2 b eye_cells, eye_at + (2 b + 2) eye_cells) of path_lists.  Jitter and the
// col_x / row_y axes are shared: the cameras of a batch have the same screen.
constexpr int kBatchMax = 8;
struct BatchView
{
    double cam[kBatchMax][15];        // Camera of every frame (FrameView::cam is frame 0's)
    trt_rayfamily eye[kBatchMax][2];  // families 0 and 1 of every frame (GridView::eye is frame 0's)
    unsigned frames, units_per_frame; // units_per_frame = owned pixels * spp
    unsigned frame_magic, reserved;   // min(ceil(2^32 / units_per_frame), 2^32 - 1): unit -> frame by multiply-high
};
constexpr size_t kArgBatch = (kArgGrids + sizeof(GridView) + alignof(BatchView) - 1) / alignof(BatchView) * alignof(BatchView);
static_assert(kArgBatch + sizeof(BatchView) <= 4096, "the arguments of a BATCH launch fit the 4 KB kernarg segment");
static_assert(sizeof(BatchView::cam) % 8 == 0 && offsetof(BatchView, eye) == sizeof(BatchView::cam) && offsetof(BatchView, frames) % 8 == 0,
              "BatchView is read as whole 64-bit words");
// A lane's frame of the batch lives as long as its sample: in the three bits above the bounce count, not in a register of its own
constexpr int kBatchFrameShift = 28;
constexpr int kBatchBounceMask = (1 << kBatchFrameShift) - 1; // a batch launch takes bounce limits up to this
static_assert(kBatchMax <= 8, "three bits of `bounces` hold the frame");
// A pointer that was read from memory is "generic" to the compiler: loads and stores through it would be FLAT instructions.
// Every pointer in the argument structs is a device-memory address: say so (a round trip through the global address space,
// from which the compiler's address-space inference takes it).
template <class T>
TRT_DEV T *in_device_memory(T *p)
{
    T __attribute__((address_space(1))) *g = (T __attribute__((address_space(1))) *)p;
    asm("" : "+s"(g)); // keeps the pair of casts from being folded back into the generic pointer
    return (T *)g;
}
TRT_DEV SceneView in_device_memory(SceneView v)
{
    v.spheres = in_device_memory(v.spheres), v.dir_lights = in_device_memory(v.dir_lights), v.point_lights = in_device_memory(v.point_lights);
    v.sky = in_device_memory(v.sky);
    return v;
}
TRT_DEV CullView in_device_memory(CullView v)
{
    v.table = in_device_memory(v.table);
    return v;
}
TRT_DEV FrameView in_device_memory(FrameView v)
{
    v.jitter = in_device_memory(v.jitter), v.col_x = in_device_memory(v.col_x), v.row_y = in_device_memory(v.row_y);
    v.samples = in_device_memory(v.samples), v.out = in_device_memory(v.out), v.ior = in_device_memory(v.ior);
    v.counters = in_device_memory(v.counters), v.queue = in_device_memory(v.queue);
    return v;
}
TRT_DEV GridView in_device_memory(GridView v)
{
    v.dir = in_device_memory(v.dir), v.point = in_device_memory(v.point);
    v.dir_lists = in_device_memory(v.dir_lists), v.point_lists = in_device_memory(v.point_lists);
    v.path_lists = in_device_memory(v.path_lists), v.pool = in_device_memory(v.pool), v.sphere_fam = in_device_memory(v.sphere_fam);
    v.patch_rec = in_device_memory(v.patch_rec);
    return v;
}
#define TRT_FRESH_ARGS                                                                             \
    const char CONSTANT_AS *fresh_ = (const char CONSTANT_AS *)__builtin_amdgcn_kernarg_segment_ptr(); \
    asm volatile("" : "+s"(fresh_));                                                               \
    const SceneView s = in_device_memory(load_kernel_argument<SceneView>(fresh_ + kArgScene));     \
    const CullView cull = in_device_memory(load_kernel_argument<CullView>(fresh_ + kArgCull));     \
    const FrameView f = in_device_memory(load_kernel_argument<FrameView>(fresh_ + kArgFrame));     \
    const GridView grids = in_device_memory(load_kernel_argument<GridView>(fresh_ + kArgGrids));   \
    const int n = s.num_spheres, nd = s.num_dir, nl = s.num_dir + s.num_point;                     \
    const unsigned pixels_here = (unsigned)f.local_rows * (unsigned)f.width;                       \
    const unsigned total = pixels_here * (unsigned)f.spp;                                          \
    const d3 gp = load3(s.ground), gn = load3(s.ground + 3);                                       \
    (void)n, (void)nd, (void)nl, (void)total, (void)pixels_here, (void)gp, (void)gn, (void)cull, (void)grids

// what the hand-out of a BATCH launch needs of the fifth argument: three scalars
struct alignas(8) BatchShape
{
    unsigned frames, units_per_frame, frame_magic, reserved;
};
TRT_DEV BatchShape load_batch_shape()
{
    const char CONSTANT_AS *args = (const char CONSTANT_AS *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(args));
    return load_kernel_argument<BatchShape>(args + kArgBatch + offsetof(BatchView, frames));
}

// The LDS image of a BATCH launch: the single-frame image with a camera block and a pair of eye families per frame.  Every
// thread reads its words of the fifth argument through the constant address space (a vector load: the index is the thread's).
TRT_DEV LdsImage stage_lds_image_batch(double *lds, const SceneView &s, const CullView &cull, const FrameView &f, const GridView &grids)
{
    const int frames = (int)load_batch_shape().frames;
    const ImageParts p = image_layout(lds, s.num_spheres, s.num_dir, s.num_point, cull.padded, f.spp, frames);
    fill_image(p, s, cull, f, grids); // frame 0's camera and families are FrameView's and GridView's; all of them follow
    const double CONSTANT_AS *cams = (const double CONSTANT_AS *)((const char CONSTANT_AS *)__builtin_amdgcn_kernarg_segment_ptr() + kArgBatch);
    const double CONSTANT_AS *eyes = cams + sizeof(BatchView::cam) / sizeof(double);
    for (int i = threadIdx.x; i < frames * kLdsCameraDoubles; i += blockDim.x)
    {
        const int b = i / kLdsCameraDoubles, j = i - b * kLdsCameraDoubles;
        const double CONSTANT_AS *c = cams + b * 15;
        // as fill_image forms them: the camera's first twelve doubles, -screen_distance, basis z * -screen_distance (TRT.c:989, :1000-1002)
        p.cam[i] = j < 12 ? c[j] : (j == 12 ? -c[12] : c[6 + (j - 13)] * -c[12]);
    }
    if (grids.path_enabled)
        for (int i = threadIdx.x; i < frames * 2 * TRT_RAYFAMILY_DOUBLES; i += blockDim.x)
            p.eye[i] = eyes[i];
    __syncthreads();
    return image_view(p);
}

#ifndef TRT_COMPACT_BLOCK
#define TRT_COMPACT_BLOCK 1024 // one workgroup per CU: 16 rings and one image share the CU's 160 KB of LDS
#endif
constexpr int kCompactBlock = TRT_COMPACT_BLOCK;
constexpr int kBigBlock = 1024;

// PATCHES: the path rays' tables have a family per PATCH of a sphere's surface (GridView::patch_m > 0, trt_raygrid.h) instead of
// one per sphere: another look-up (path_cell_patches), the same everything else.  Its own instantiation, so that scenes
// without patches run the code -- and the register allocation -- they ran before there were any.
// BIG (round 5): the plain rounds in workgroups of 1024 threads -- ONE LDS image per CU, shared by sixteen waves -- for scenes whose
// image no longer fits four times into a CU's 160 KB (above ~290 spheres: 136 bytes a sphere): with 256-thread workgroups such a
// scene runs three, two, one wave per SIMD (512 spheres: two).  Same code; the register allocator has to stay under 128.
// DEVICE_IMAGE: the scene image is not staged into LDS but read from f.image, where stage_image_kernel (trt_render.hip) wrote it
// for this launch in the same layout: scenes whose image does not fit LDS.  No dynamic LDS; the plain rounds only.
// BATCH: several frames of one scene per launch (BatchView above); the launch has a fifth argument, `batch`, a BatchView, which the
// kernel reads where it needs it (stage_lds_image_batch, load_batch_shape).  Every difference is behind `if constexpr (BATCH)` or a
// constant that folds: the single-frame instantiations are what they were.
// SPECULAR (EXTENSION, parity unpinned, trt_set_specular): the lights' Blinn-Phong terms (shadow_stage), on the plain rounds with or
// without patches.  A task of the decoupled ring would have to carry the view vector, three more doubles: not built.  Its register
// budget is four waves per SIMD: left at three the allocator took 137 VGPRs for the instantiation without patches -- three waves -- and
// the term cost config 2 45 % of a frame instead of 24 (profiles/r25/a_specular.md); asked for four it settles at 126, nothing spilt.
// SKY_FILTER (EXTENSION, parity unpinned, trt_set_sky_filter): a sample that ends on the sky takes the bilinear blend of four texels
// (sky_filtered_wave / sky_blend, trt_device.hpp) where the others take the nearest one, on the plain rounds with or without patches.
// The round carries the four words and the two weights from the loads to the END of the bounce, seven registers more than the one
// word; the FP64 coordinates are always formed, there is no FP32 estimate of a weight.  Its register budget is the plain rounds' -- the
// launch bound is left at TRT_ROUNDS_WAVES, and the allocator settles at 124 / 125 VGPRs, four waves a SIMD like its twins (118 / 119).
// NOTHING IN THE LAUNCH BOUND HOLDS IT THERE: a change that takes the instantiations without counters above 128 drops them to three
// waves, as the specular term did at 137 before it asked for four.  The Makefile prints their VGPRs beside render_rounds_kernel<false>'s
// and warns above 128; asking for four waves outright has not been measured against this.
template <bool COUNT, bool REFRACT = false, bool COMPACT = false, bool PATCHES = false, bool BIG = false, bool DEVICE_IMAGE = false, bool BATCH = false,
          bool SPECULAR = false, bool SKY_FILTER = false, class... BatchArgument>
__global__ __launch_bounds__(BIG ? kBigBlock : COMPACT ? kCompactBlock : kPersistentBlock, ((COMPACT && !COUNT) || BIG || (SPECULAR && !COUNT) /* 126 / 127 VGPRs asked for four waves, 137 left at three */) ? 4 : TRT_ROUNDS_WAVES) void render_rounds_kernel(SceneView s, CullView cull, FrameView f, GridView grids, BatchArgument... batch)
{
    static_assert(sizeof...(BatchArgument) == (BATCH ? 1 : 0), "a BATCH launch has one more argument, a BatchView; the others none");
    static_assert(!BATCH || (!COUNT && !REFRACT && !BIG && !DEVICE_IMAGE), "several frames per launch: the plain, patch and decoupled rounds");
    static_assert(!(REFRACT && COMPACT), "the refraction extension runs on the plain rounds");
    static_assert(!(PATCHES && COMPACT), "scenes with patches run the plain rounds");
    static_assert(!BIG || (PATCHES && !COUNT && !REFRACT && !COMPACT), "1024-thread workgroups: the shipping patch instantiation only");
    static_assert(!DEVICE_IMAGE || (!REFRACT && !COMPACT && !BIG), "the device-memory image: the plain rounds only");
    static_assert(!SPECULAR || (!COMPACT && !BIG && !DEVICE_IMAGE && !BATCH && !REFRACT), "the specular extension: the plain rounds with the image in LDS, one frame a launch");
    static_assert(!SKY_FILTER || (!COMPACT && !BIG && !DEVICE_IMAGE && !BATCH && !REFRACT && !SPECULAR), "bilinear sky filtering: the plain rounds with the image in LDS, one frame a launch, no other extension");
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const LdsImage L = BATCH ? stage_lds_image_batch(lds, s, cull, f, grids)
                       : DEVICE_IMAGE ? image_view(image_layout(const_cast<double *>(f.image), s.num_spheres, s.num_dir, s.num_point, cull.padded, f.spp))
                                      : stage_lds_image(lds, s, cull, f, grids);
    const int n = s.num_spheres, nd = s.num_dir, nl = s.num_dir + s.num_point;
    const int lane = threadIdx.x & 63;
    const unsigned pixels_here = (unsigned)f.local_rows * (unsigned)f.width;
    const unsigned total = pixels_here * (unsigned)f.spp; // work units, < 2^31
    (void)total; // TRT_FRESH_ARGS re-derives it where it is used
    const d3 gp = load3(s.ground), gn = load3(s.ground + 3);

    // ---- per-lane state ------------------------------------------------------------------------------
    bool alive = true;             // owns a unit (a sample being traced)
    bool want_unit = true;         // needs a (new) unit before the next round
    unsigned slot_id = 0;          // k*pixels + pixel: where the sample's colour goes in f.samples
    d3 sample = d3{0.0, 0.0, 0.0}; // pixel_color of the sample (TRT.c:1012)
    double weight = 1.0, weight_sum = 0.0;
    int bounces = 0;               // BATCH: the sample's frame of the batch in the bits from kBatchFrameShift up
    d3 o = d3{0.0, 0.0, 0.0}, d = d3{0.0, 0.0, -1.0}; // the pending path ray
    d3 next_dir = d;                                  // un-normalised direction of the next path ray
    int fam = 0;                                      // family of the pending path ray (trt_raygrid.h): 0 = it starts at the eye
    int inside = -1;                                  // REFRACT: the refractor the pending ray travels inside of
    Tally tally;
    unsigned pool_next = 0, pool_end = 0; // wave-uniform: units fetched from the queue, not yet handed out
    { // the queue (trt_common.hpp, kQueueStride): the first chunk is the wave's own -- 4096 waves asking for their first units at the
      // same moment would wait in line for them
        const unsigned group = blockIdx.x, waves = blockDim.x >> 6, wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const unsigned j = (group >> f.queue_shift) * waves + wave;
        pool_next = ((j << f.queue_shift) + (group & ((1u << f.queue_shift) - 1u))) * f.chunk;
        pool_end = pool_next + f.chunk;
    }
    // COMPACT: the wave's ring of shading tasks and what this lane still expects from it
    double *const ring = lds + f.ring_at + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * kRingDoubles; // wave-uniform: a scalar
    unsigned short *const ring_mat = (unsigned short *)(ring + 7 * kRingTasks); // < 2^16 materials: the LDS image ends long before
    double *const parked = ring + 7 * kRingTasks + kRingTasks / 4;
    if (COMPACT)
    {
        for (int i = lane; i < kRingDoubles; i += 64)
            ring[i] = 0.0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    unsigned q_head = 0, q_tail = 0, q_old = 0; // wave-uniform counters: [q_head, q_tail) waits, tasks below q_old are of the previous round
    unsigned my_task = 0, old_slot = 0;         // this round's task of the lane (its number), the previous round's (its place in the ring)
    bool my_open = false, old_open = false;     // ... whose colour has not arrived yet
    bool waiting = false;                       // the sample ended on a hit whose colour arrives in the next round: the lane sits that round out
    for (;;)
    {
        TRT_MARK_AT(22); // loop edge
        // =============== hand out work units; primary rays of new samples (TRT.c:981-1016) ===============
        {
            TRT_FRESH_ARGS;
            const unsigned long long need = __ballot(want_unit);
            if (need)
            {
                const unsigned wanted = (unsigned)__builtin_popcountll(need);
                const unsigned rank = lanes_below(need);
                unsigned mine = pool_next + rank;
                if (pool_end - pool_next < wanted)
                { // refill the wave's pool with ONE atomic; what is left of the old chunk is served first
                    const unsigned left = pool_end - pool_next;
                    unsigned fresh = 0;
                    const int leader = __builtin_ctzll(need);
                    const unsigned word = blockIdx.x & ((1u << f.queue_shift) - 1u); // the workgroup's word of the queue: its XCD's
                    if (lane == leader)
                        fresh = atomicAdd(f.queue + word * kQueueStride, 1u);
                    fresh = (unsigned)__builtin_amdgcn_readlane((int)fresh, leader); // the leader is wave-uniform: no cross-lane permute, no lane id
                    fresh = ((fresh << f.queue_shift) + word) * f.chunk; // a chunk of this launch or one of the first few behind its end: < 2^32
                    if (rank >= left)
                        mine = fresh + (rank - left);
                    pool_next = fresh + (wanted - left);
                    pool_end = fresh + f.chunk;
                }
                else
                    pool_next += wanted;
                BatchShape shape{};
                if constexpr (BATCH)
                    shape = load_batch_shape();
                if (want_unit)
                {
                    alive = mine < (BATCH ? shape.frames * total : total); // BATCH: `total` is one frame's units
                    if (alive)
                    {
                        // unit -> (pixel, k) -> (row, column) by multiply-high with min(ceil(2^32/x), 2^32-1): off by at most one
                        // either way; the correction is two selects each, not branches (three nested exec regions per lane before)
                        unsigned frame = 0;
                        if constexpr (BATCH)
                        { // unit -> (frame, unit of the frame) in the same way, first: lanes of one wave may be in different frames
                            frame = __umulhi(mine, shape.frame_magic);
                            const int within = (int)(mine - frame * total); // in (-total, 2 total): no overflow, frames * total < 2^31
                            const int under = within < 0, over = within >= (int)total;
                            frame += (unsigned)(over - under);
                            mine = (unsigned)(within + (under - over) * (int)total);
                        }
                        const double *const cam = L.cam + (BATCH ? frame * (unsigned)kLdsCameraDoubles : 0u);
                        unsigned pixel = __umulhi(mine, f.spp_magic);
                        int k = (int)(mine - pixel * (unsigned)f.spp);
                        {
                            const int under = k < 0, over = k >= f.spp;
                            pixel += (unsigned)(over - under);
                            k += (under - over) * f.spp;
                        }
                        slot_id = (unsigned)k * pixels_here + pixel; // sample-major scratch: the reduction streams it
                        unsigned row = __umulhi(pixel, f.width_magic);
                        int col = (int)(pixel - row * (unsigned)f.width);
                        {
                            const int under = col < 0, over = col >= f.width;
                            row += (unsigned)(over - under);
                            col += (under - over) * f.width;
                        }
                        const double sx = f.col_x[col] + L.jit[k];
                        // rows dealt from tile 0 with step 1 (a whole frame, a one-rank shard): the local row IS the frame row
                        const double sy = f.row_y[f.tile_first == 0 && f.tile_step == 1 ? (int)row : frame_row_of_magic(f, row)] + L.jit[f.spp + k];
                        d3 dir = d3{0.0, 0.0, 0.0};
                        dir = add(dir, scale(load3(cam + 0), sx));
                        dir = add(dir, scale(load3(cam + 3), sy));
                        dir = add(dir, load3(cam + 13)); // scale(basis z, sz), formed once per workgroup (stage_lds_image)
                        next_dir = sub(dir, load3(cam + 9)); // sic, TRT.c:1005
                        o = load3(cam + 9);
                        fam = 0;
                        inside = -1;
                        sample = d3{0.0, 0.0, 0.0};
                        weight = 1.0;
                        weight_sum = 0.0;
                        bounces = BATCH ? (int)(frame << kBatchFrameShift) : 0;
                    }
                    want_unit = false;
                }
            }
        }
        const unsigned long long alive_lanes = lanes_with(alive); // the round's votes AND their compares into it (trt_device.hpp, lanes_with)
        if ((COMPACT ? alive_lanes | lanes_with(waiting) : alive_lanes) == 0)
            break;
        if (COUNT)
            tally.rounds++;
        TRT_MARK_AT(0); // units + primary rays
        bool d_plain; // the wave's directions are unit vectors by construction (unit_round, trt_device.hpp)
        d = unit_round(next_dir, d_plain); // TRT.c:1008 for a primary ray, TRT.c:1055 for a reflected one

        // ======================================= P: the path ray =======================================
        if (COUNT && alive)
            tally.path++;
        TRT_MARK_AT(1); // unit(next_dir)
        PathHit hit;
        {
            TRT_FRESH_ARGS;
            hit = path_stage<COUNT, REFRACT, PATCHES, BATCH>(L, cull, grids, n, o, d, fam, alive, alive_lanes, gp, gn, tally, inside, BATCH ? bounces >> kBatchFrameShift : 0, d_plain);
        }
        if constexpr (COMPACT)
        {
            const bool path_hit = hit.hit, path_sky = hit.sky;
            bool end_sample = path_sky;
            uint32_t sky_t = 0;
            const double weight_before = weight;
            {
            TRT_FRESH_ARGS;
            if (hit.sky_lanes != 0)
                sky_t = sky_texel_wave(s.sky, s.sky_dim, hit.back, s.sky_dim_f, path_sky, hit.sky_lanes); // TRT.c:858-867; added to the sample after the colours still on their way
            // ---- a hit becomes a task; what does not depend on its colour happens now (TRT.c:1036-1038, :1054) ----
            const unsigned long long hits = hit.hit_lanes;
            if (hits)
            {
                if (path_hit)
                {
                    my_task = q_tail + lanes_below(hits);
                    my_open = true;
                    const unsigned at = my_task & (kRingTasks - 1);
                    const d3 so = add(hit.ph.p, scale(hit.back, 0.000001)); // TRT.c:873-874
                    ring[0 * kRingTasks + at] = so.x, ring[1 * kRingTasks + at] = so.y, ring[2 * kRingTasks + at] = so.z;
                    ring[3 * kRingTasks + at] = hit.normal.x, ring[4 * kRingTasks + at] = hit.normal.y, ring[5 * kRingTasks + at] = hit.normal.z;
                    ring[6 * kRingTasks + at] = weight;
                    ring_mat[at] = (unsigned short)hit.mat;
                    const d3 nd3 = reflect(d, hit.normal); // TRT.c:1054; kept in LDS while the wave shades
                    parked[lane] = nd3.x, parked[64 + lane] = nd3.y, parked[128 + lane] = nd3.z;
                    weight *= L.mat[hit.mat * 5 + 3];
                    bounces++;
                    end_sample = !((BATCH ? bounces & kBatchBounceMask : bounces) < f.bounce_limit && weight > 0.00001); // TRT.c:1018
                }
                q_tail += (unsigned)__builtin_popcountll(hits);
            }
            }
            if (alive)
                weight_sum += weight_before; // TRT.c:1034 (a sample that ends is normalised by this sum, one that goes on carries it)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // the ring is written by some lanes and read by others
            TRT_MARK_AT(7); // P post: sky texel, reflection, nudge, enqueue
            // ---- S over tasks: ONE pass of up to 64 tasks from the head of the ring, if a task of the previous round waits (they
            // are at the head, fewer than 64) or 64 wait.  At most 63 stay behind, so 63 + 64 is the most the ring ever holds. ----
            if (q_head != q_tail && ((int)(q_old - q_head) > 0 || q_tail - q_head >= 64u))
            {
                TRT_FRESH_ARGS;
                const unsigned take = q_tail - q_head < 64u ? q_tail - q_head : 64u;
                const bool has = (unsigned)lane < take;
                const unsigned at = (q_head + (unsigned)lane) & (kRingTasks - 1);
                // lanes beyond `take` read whatever their slot holds -- an old task or the zeros the ring started with -- and
                // take no part in the stage (lit_lanes = has); nothing they compute is stored
                const d3 so = d3{ring[0 * kRingTasks + at], ring[1 * kRingTasks + at], ring[2 * kRingTasks + at]};
                const d3 sn = d3{ring[3 * kRingTasks + at], ring[4 * kRingTasks + at], ring[5 * kRingTasks + at]};
                const int sm = ring_mat[at];
                if (COUNT)
                    tally.passes++;
                const d3 lit = shadow_stage<COUNT>(L, cull, grids, n, nd, nl, so, sn, sm, has, lanes_with(has), gp, gn, tally);
                d3 color = d3{clampd(lit.x, 0.0, 1.0), clampd(lit.y, 0.0, 1.0), clampd(lit.z, 0.0, 1.0)}; // TRT.c:960-962
                color = scale(color, ring[6 * kRingTasks + at]);                                          // TRT.c:1035
                if (has) // the colour takes the place of the normal in the task's record; its owner collects it at the END of a round
                    ring[3 * kRingTasks + at] = color.x, ring[4 * kRingTasks + at] = color.y, ring[5 * kRingTasks + at] = color.z;
                q_head += take;
            }
            q_old = q_tail;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            TRT_MARK_AT(20); // lit accumulate
            // ---- colours that have arrived, in bounce order (TRT.c:1040): last round's task is shaded by now, this round's may be ----
            if (old_open)
            {
                const unsigned at = old_slot;
                sample = add(sample, d3{ring[3 * kRingTasks + at], ring[4 * kRingTasks + at], ring[5 * kRingTasks + at]});
            }
            if (my_open && (int)(q_head - my_task) > 0)
            {
                const unsigned at = my_task & (kRingTasks - 1);
                sample = add(sample, d3{ring[3 * kRingTasks + at], ring[4 * kRingTasks + at], ring[5 * kRingTasks + at]});
                my_open = false;
            }
            // ======================================= END of the bounce =======================================
            if (path_hit)
            { // the next path ray: from the nudged point, along the reflection
                o = d3{ring[0 * kRingTasks + (my_task & (kRingTasks - 1))], ring[1 * kRingTasks + (my_task & (kRingTasks - 1))],
                       ring[2 * kRingTasks + (my_task & (kRingTasks - 1))]};
                next_dir = d3{parked[lane], parked[64 + lane], parked[128 + lane]};
            }
            // A sample that ended on this round's hit while the hit's colour is still on its way waits for it: the lane sits
            // the next round out (its task is then of the previous round: shaded whatever else happens) and stores the sample at
            // that round's END.
            bool finish = end_sample;
            if (waiting)
                finish = true, waiting = false; // the colour it waited for was added above
            else if (end_sample && my_open)
                finish = false, waiting = true, alive = false;
            old_slot = my_task & (kRingTasks - 1), old_open = my_open, my_open = false;
            if (path_sky)
            { // TRT.c:1044-1048: colour = texel, the sample ends here
                const d3 color = d3{L.b255[sky_t & 0xFF], L.b255[(sky_t >> 8) & 0xFF], L.b255[(sky_t >> 16) & 0xFF]};
                sample = add(sample, scale(color, weight));
            }
            if (__any(finish))
            { // TRT.c:1061
                const double q = 1.0 / weight_sum;
                if (finish)
                {
                    TRT_FRESH_ARGS;
                    unsigned slot = slot_id;
                    asm volatile("" : "+v"(slot)); // the address is formed here, not kept as 64 bits for the life of the sample
                    double *out = f.samples + (size_t)slot * 3;
                    if constexpr (BATCH) // scratch [frame][k][pixel][3]: the slot is the frame's, the frame's offset 64 bits
                        out += (size_t)(unsigned)(bounces >> kBatchFrameShift) * total * 3;
                    out[0] = sample.x * q;
                    out[1] = sample.y * q;
                    out[2] = sample.z * q;
                    want_unit = true;
                }
            }
        }
        else
        {
        // REFRACT: the ray leaves the refractor it was inside of -- no shading, no weight, one bounce
        const bool leaving = REFRACT && hit.hit && hit.ph.i == inside;
        const bool path_hit = hit.hit && !leaving, path_sky = hit.sky;
        const d3 h_normal = hit.normal;
        const int h_mat = hit.mat;
        bool end_sample = false;
        double weight_sum_new = weight_sum + weight; // TRT.c:1034
        uint32_t sky_t = 0;
        [[maybe_unused]] SkyTaps sky_taps{}; // SKY_FILTER: the four texels and the two weights in sky_t's place
        if (hit.sky_lanes != 0)
        { // TRT.c:858-867, :1044-1048: colour = texel, the sample ends here.  The texel is only LOADED here: it is a dependent read
          // from global memory, and what uses it (the sample's colour) is not needed before the END of the round, behind the other
          // lanes' shadow stages
            TRT_FRESH_ARGS;
            if constexpr (SKY_FILTER)
                sky_taps = sky_filtered_wave(s.sky, s.sky_dim, hit.back, s.sky_dim_f, path_sky); // four loads, blended at the END of the round
            else
            sky_t = sky_texel_wave(s.sky, s.sky_dim, hit.back, s.sky_dim_f, path_sky, hit.sky_lanes);
            end_sample = path_sky;
        }
        d3 lit;
        if (!REFRACT)
        {
            if (path_hit)
            {
                next_dir = reflect(d, h_normal);              // TRT.c:1054, normalised at the top of the next round
                o = add(hit.ph.p, scale(hit.back, 0.000001)); // TRT.c:873-874; origin of the shadow rays and of the next path ray
            }
            TRT_MARK_AT(7); // P post: sky texel, reflection, nudge
            // ===================================== S(i): shadow rays =====================================
            if (COUNT && hit.hit_lanes != 0)
                tally.passes++;
            {
                TRT_FRESH_ARGS;
                if constexpr (SPECULAR)
                    lit = shadow_stage<COUNT, true>(L, cull, grids, n, nd, nl, o, h_normal, h_mat, path_hit, hit.hit_lanes, gp, gn, tally, scale(d, -1.0)); // TRT.c:1029
                else
                lit = shadow_stage<COUNT>(L, cull, grids, n, nd, nl, o, h_normal, h_mat, path_hit, hit.hit_lanes, gp, gn, tally); // !REFRACT: path_hit is hit.hit
            }
        }
        else
        {
            const d3 shade_at = add(hit.ph.p, scale(hit.back, 0.000001)); // TRT.c:873-874: where the surface is lit; origin of a reflected ray
            if (hit.hit)
            {
                bool bent = false;
                if (hit.ph.i < n)
                {
                    const double ior = f.ior[hit.ph.i];
                    if (ior > 0.0)
                    {
                        const d3 nn = leaving ? scale(h_normal, -1.0) : h_normal; // the normal facing the incoming ray
                        const double cosi = -dot(nn, d);
                        const double eta = leaving ? ior : 1.0 / ior;
                        const double kk = 1.0 - (eta * eta) * (1.0 - cosi * cosi);
                        bent = true;
                        if (!(kk < 0.0))
                        {
                            const double fac = eta * cosi - __builtin_sqrt(kk);
                            next_dir = d3{eta * d.x + fac * nn.x, eta * d.y + fac * nn.y, eta * d.z + fac * nn.z};
                            o = sub(hit.ph.p, scale(hit.back, 0.000001)); // 1e-6 past the surface
                            inside = leaving ? -1 : hit.ph.i;
                        }
                        else
                        { // total internal reflection: mirror about the facing normal, stay on this side
                            next_dir = reflect(d, nn);
                            o = shade_at;
                        }
                    }
                }
                if (!bent)
                {
                    next_dir = reflect(d, h_normal);
                    o = shade_at;
                }
            }
            lit = shadow_stage<COUNT>(L, cull, grids, n, nd, nl, shade_at, h_normal, h_mat, path_hit, lanes_with(path_hit), gp, gn, tally);
        }

        TRT_MARK_AT(20); // lit accumulate
        // ======================================= END of the bounce =======================================
        if (path_hit)
        { // TRT.c:960-962 then :1034-1048
            TRT_FRESH_ARGS;
            d3 color = d3{clampd(lit.x, 0.0, 1.0), clampd(lit.y, 0.0, 1.0), clampd(lit.z, 0.0, 1.0)};
            color = scale(color, weight);
            weight *= L.mat[h_mat * 5 + 3];
            bounces++;
            sample = add(sample, color);
            if ((BATCH ? bounces & kBatchBounceMask : bounces) < f.bounce_limit && weight > 0.00001) // TRT.c:1018
                weight_sum = weight_sum_new;
            else
                end_sample = true;
        }
        if (REFRACT && leaving)
        {
            bounces++;
            weight_sum_new = weight_sum; // nothing was contributed
            if (!(bounces < f.bounce_limit))
                end_sample = true;
        }
        if (path_sky)
        { // TRT.c:866, :1035-1051: colour = texel / 255, scaled by the sample's weight
            d3 color;
            if constexpr (SKY_FILTER)
                color = sky_blend(sky_taps);
            else
                color = d3{L.b255[sky_t & 0xFF], L.b255[(sky_t >> 8) & 0xFF], L.b255[(sky_t >> 16) & 0xFF]};
            sample = add(sample, scale(color, weight));
        }
        if (__any(end_sample))
        { // TRT.c:1061: the sample's colour, normalised by the weights it gathered
            const double q = 1.0 / weight_sum_new;
            if (end_sample)
            {
                TRT_FRESH_ARGS;
                double *out = f.samples + (size_t)slot_id * 3;
                if constexpr (BATCH) // scratch [frame][k][pixel][3]
                    out += (size_t)(unsigned)(bounces >> kBatchFrameShift) * total * 3;
                out[0] = sample.x * q; // plain stores: non-temporal ones (keeping the 498 MB stream out of L2) measured no different
                out[1] = sample.y * q;
                out[2] = sample.z * q;
                want_unit = true;
            }
        }
        }
        TRT_MARK_AT(21); // END of the bounce
    }

#if defined(TRT_MARKS) && TRT_MARKS == 2
    // ISA profile (tools/isa_profile.py): lane `slot` of v240 + kind holds the wave's executed instructions of that kind in
    // the intervals that START at stage boundary `slot` (63: before the first boundary)
    if (!COUNT && f.counters)
    {
#define TRT_PROFILE_DUMP(kind)                                                         \
    {                                                                                  \
        unsigned x_;                                                                   \
        asm volatile("v_mov_b32 %0, v" #kind : "=v"(x_));                              \
        atomicAdd(&f.counters[kProfileAt + 64 * ((kind) - 240) + lane], (unsigned long long)x_); \
    }
        TRT_PROFILE_DUMP(240) TRT_PROFILE_DUMP(241) TRT_PROFILE_DUMP(242) TRT_PROFILE_DUMP(243) TRT_PROFILE_DUMP(244) TRT_PROFILE_DUMP(245)
        TRT_PROFILE_DUMP(246) TRT_PROFILE_DUMP(247) TRT_PROFILE_DUMP(248) TRT_PROFILE_DUMP(249) TRT_PROFILE_DUMP(250)
#undef TRT_PROFILE_DUMP
    }
#endif
    if (COUNT && f.counters)
    {
        atomicAdd(&f.counters[0], (unsigned long long)tally.path);
        atomicAdd(&f.counters[1], (unsigned long long)tally.shadow);
        for (int k = 0; k < 3; k++)
            atomicAdd(&f.counters[33 + k], (unsigned long long)tally.tests[k]); // exact tests per lane: tests / (64 iterations) = lane activity
        if (lane == 0)
        {
            atomicAdd(&f.counters[2], (unsigned long long)tally.rounds);
            atomicAdd(&f.counters[3], (unsigned long long)tally.iters[0] + tally.iters[1] + tally.iters[2]);
            atomicAdd(&f.counters[28], (unsigned long long)tally.swept); // traces in which the wave fell back to the sweep
            atomicAdd(&f.counters[29], (unsigned long long)tally.passes); // times the wave ran the shadow stage
            for (int k = 0; k < 3; k++)
                atomicAdd(&f.counters[30 + k], (unsigned long long)tally.iters[k]); // wave-level iterations of the three exact-test loops
            atomicAdd(&f.counters[36], (unsigned long long)tally.full);            // point-light searches that fell back to the closest hit
        }
    }
}

// trt_probe_rays through the PRODUCTION stages: one lane per ray, the very path_stage / shadow_stage of the render kernel
// (tables, fall-back sweep, exact tests, lighting).  families[i]: the family ray i is looked up in (trt_raygrid.h; < 0: none,
// the wave sweeps); nullptr: none for every ray.  Outputs as trace_ray / apply_lighting produce them (TRT.c:793-963).
// SPECULAR: the context's specular extension is on (trt_set_specular); lit_out then holds the clamped colour with the lights' terms,
// the view vector being minus the ray's direction as it was given.
// SKY_FILTER: the context's sky filter is bilinear (trt_set_sky_filter); a miss's material colour is then the blend of the four taps.
template <bool PATCHES, bool SPECULAR = false, bool SKY_FILTER = false>
__global__ __launch_bounds__(kPersistentBlock) void probe_rounds_kernel(SceneView s, CullView cull, FrameView f, GridView grids, const double *rays,
                                                                        const int *families, long count, int *obj, double *point, double *normal,
                                                                        double *material, double *lit_out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const LdsImage L = stage_lds_image(lds, s, cull, f, grids);
    const int n = s.num_spheres, nd = s.num_dir, nl = s.num_dir + s.num_point;
    const d3 gp = load3(s.ground), gn = load3(s.ground + 3);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool alive = i < count;
    const long at = alive ? i : 0;
    const d3 o = load3(rays + 6 * at), d = load3(rays + 6 * at + 3);
    int fam = families ? families[at] : -1;
    Tally tally;
    const PathHit hit = path_stage<false, false, PATCHES>(L, cull, grids, n, o, d, fam, alive, lanes_with(alive), gp, gn, tally);
    const d3 surface = hit.hit ? add(hit.ph.p, scale(hit.back, 0.000001)) : o; // TRT.c:873-874 / :860
    d3 lit;
    if constexpr (SPECULAR)
        lit = shadow_stage<false, true>(L, cull, grids, n, nd, nl, surface, hit.normal, hit.mat, hit.hit, hit.hit_lanes, gp, gn, tally, scale(d, -1.0));
    else
        lit = shadow_stage<false>(L, cull, grids, n, nd, nl, surface, hit.normal, hit.mat, hit.hit, hit.hit_lanes, gp, gn, tally);
    uint32_t sky_t = 0;
    [[maybe_unused]] SkyTaps sky_taps{};
    if constexpr (SKY_FILTER)
        sky_taps = sky_filtered_wave(s.sky, s.sky_dim, hit.back, s.sky_dim_f, alive && !hit.hit);
    else
        sky_t = sky_texel_wave(s.sky, s.sky_dim, hit.back, s.sky_dim_f, alive && !hit.hit, hit.sky_lanes); // the render kernels' look-up
    if (!alive)
        return;
    d3 color = d3{0.0, 0.0, 0.0};
    double refl = 0.0, spec = 0.0; // TRT.c:866: the compound literal zero-fills
    d3 nrm = hit.back;             // a miss: the (normalised) ray direction, TRT.c:861, :878
    if (hit.hit)
    {
        color = load3(L.mat + hit.mat * 5);
        refl = L.mat[hit.mat * 5 + 3];
        spec = L.mat[hit.mat * 5 + 4];
        nrm = hit.normal;
    }
    else
    {
        const uint32_t t = sky_t;
        if constexpr (SKY_FILTER)
            color = sky_blend(sky_taps);
        else
            color = d3{L.b255[t & 0xFF], L.b255[(t >> 8) & 0xFF], L.b255[(t >> 16) & 0xFF]};
    }
    obj[i] = hit.hit ? (hit.ph.i < n ? 1 : 2) : 0;
    point[3 * i + 0] = surface.x, point[3 * i + 1] = surface.y, point[3 * i + 2] = surface.z;
    normal[3 * i + 0] = nrm.x, normal[3 * i + 1] = nrm.y, normal[3 * i + 2] = nrm.z;
    material[5 * i + 0] = color.x, material[5 * i + 1] = color.y, material[5 * i + 2] = color.z;
    material[5 * i + 3] = refl, material[5 * i + 4] = spec;
    const d3 c = hit.hit ? d3{clampd(lit.x, 0.0, 1.0), clampd(lit.y, 0.0, 1.0), clampd(lit.z, 0.0, 1.0)} : d3{0.0, 0.0, 0.0}; // TRT.c:960
    lit_out[3 * i + 0] = c.x, lit_out[3 * i + 1] = c.y, lit_out[3 * i + 2] = c.z;
}

} // namespace trt
