/* lightgrid_check.c -- host-side validation of the light-space candidate masks (csrc/trt_lightgrid.h).
 * Test helper only: compiled by tests/test_lightgrid.py with gcc -O2 -ffp-contract=off.
 * For every shadow ray it looks up the ray's cell exactly as the kernel does and compares with the EXACT
 * reference test (TRT.c:638-672, FP64, reference operation order) of every sphere:
 *   directional light: a sphere the exact test hits must be in the cell (a violation otherwise);
 *   point light: the same for every hit not farther than the light + near/2, and the lit/dark decision of
 *   TRT.c:936-946 taken from the cell's spheres alone must equal the decision taken from all spheres. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "trt_raygrid.h" /* the packing of list cells; it includes trt_lightgrid.h */

typedef struct
{
    unsigned long long rays, far, exact_hits, candidates, violations, decision_mismatches, bits_set, cells;
    unsigned long long wave_max_cand, wave_groups;
    unsigned long long cand_hist[17];
    double first_violation[8]; /* ray(6), sphere index, cell */
} grid_stats;

static int exact_hit(const double *o, const double *d, double a, const double *s, double *t_out)
{
    const double ocx = o[0] - s[0], ocy = o[1] - s[1], ocz = o[2] - s[2];
    const double b = 2.0 * (ocx * d[0] + ocy * d[1] + ocz * d[2]);
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - s[3] * s[3];
    const double disc = b * b - 4.0 * a * c;
    if (disc < 0.0)
        return 0;
    const double t0 = (-b - sqrt(disc)) / (2.0 * a);
    *t_out = t0;
    return t0 > 0.0;
}

static int in_cell(const unsigned long long *cell, int i) { return (cell[i >> 6] >> (63 - (i & 63))) & 1; }

static void note(grid_stats *st, const double *ray, int sphere, int cell)
{
    if (!st->violations)
    {
        memcpy(st->first_violation, ray, 6 * sizeof(double));
        st->first_violation[6] = sphere;
        st->first_violation[7] = cell;
    }
    st->violations++;
}

static void tally(grid_stats *st, unsigned cand, unsigned *group_max, size_t r, size_t n_rays)
{
    st->candidates += cand;
    st->cand_hist[cand > 16 ? 16 : cand]++;
    *group_max = cand > *group_max ? cand : *group_max;
    if ((r & 63) == 63 || r + 1 == n_rays)
    {
        st->wave_max_cand += *group_max;
        st->wave_groups++;
        *group_max = 0;
    }
}

/* all rays share the direction rays[3..5] (the unit to-light vector) */
void dirgrid_check(const double *spheres, int n, const double *rays, size_t n_rays, int g, int slabs, grid_stats *st)
{
    memset(st, 0, sizeof *st);
    if (!n_rays)
        return;
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    const int words = (n + 63) / 64 > 0 ? (n + 63) / 64 : 1;
    if (slabs < 1)
        slabs = 1;
    unsigned long long *masks = (unsigned long long *)malloc(sizeof(unsigned long long) * (size_t)slabs * g * g * words);
    trt_dirgrid G;
    trt_dirgrid_disc *discs = (trt_dirgrid_disc *)malloc(sizeof(trt_dirgrid_disc) * (size_t)(n ? n : 1));
    st->bits_set = (unsigned long long)trt_dirgrid_build(spheres, n, &cs, rays + 3, g, slabs, &G, masks, discs);
    free(discs);
    st->cells = (unsigned long long)slabs * g * g;
    /* the clamp relies on an empty border */
    for (int s = 0; s < slabs; s++)
        for (int j = 0; j < g; j++)
            for (int c = 0; c < g; c++)
                if (j == 0 || c == 0 || j == g - 1 || c == g - 1)
                    for (int w = 0; w < words; w++)
                        if (masks[(((size_t)s * g + j) * g + c) * words + w])
                            st->violations += 1000000;
    unsigned group_max = 0;
    for (size_t r = 0; r < n_rays; r++)
    {
        const double *o = rays + 6 * r, *d = o + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        int far;
        const int cell = trt_dirgrid_cell(&G, o[0], o[1], o[2], &far);
        st->rays++;
        if (far || !(fabs(a - 1.0) <= 9.094947017729282e-13))
        {
            st->far++;
            continue;
        }
        if (cell < 0 || cell >= slabs * g * g)
        {
            note(st, o, -1, cell);
            continue;
        }
        const unsigned long long *m = masks + (size_t)cell * words;
        unsigned cand = 0;
        for (int i = 0; i < n; i++)
        {
            double t;
            const int hit = exact_hit(o, d, a, spheres + 9 * i, &t);
            st->exact_hits += hit;
            cand += in_cell(m, i);
            if (hit && !in_cell(m, i))
                note(st, o, i, cell);
        }
        tally(st, cand, &group_max, r, n_rays);
    }
    free(masks);
    free(table);
}

/* squared distance from o to the hit point nudged back along the ray, formed as TRT.c:871-874 and :939-942 do */
static double nudged_d2(const double *o, const double *d, double t)
{
    const double p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    double back[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
    const double l = sqrt(back[0] * back[0] + back[1] * back[1] + back[2] * back[2]);
    double q[3];
    for (int k = 0; k < 3; k++)
        q[k] = (p[k] + (back[k] / l) * 0.000001) - o[k];
    return q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
}

/* lit/dark from the closest hit among the spheres selected by `m` (NULL = all), TRT.c:808-820 and :936-946 */
static int decide_lit(const double *spheres, int n, const unsigned long long *m, const double *o, const double *d, double a, double light_d2)
{
    double best_d2 = INFINITY, best_t = 0.0;
    int best = -1;
    for (int i = 0; i < n; i++)
    {
        if (m && !in_cell(m, i))
            continue;
        double t;
        if (!exact_hit(o, d, a, spheres + 9 * i, &t))
            continue;
        const double p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        const double d2 = (o[0] - p[0]) * (o[0] - p[0]) + (o[1] - p[1]) * (o[1] - p[1]) + (o[2] - p[2]) * (o[2] - p[2]);
        if (d2 < best_d2)
            best_d2 = d2, best = i, best_t = t;
    }
    if (best < 0)
        return 1;
    return light_d2 < nudged_d2(o, d, best_t);
}

void pointgrid_check(const double *spheres, int n, const double *light, const double *rays, size_t n_rays, int g, int shells, grid_stats *st)
{
    memset(st, 0, sizeof *st);
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    const int words = (n + 63) / 64 > 0 ? (n + 63) / 64 : 1;
    if (shells < 1)
        shells = 1;
    unsigned long long *masks = (unsigned long long *)malloc(sizeof(unsigned long long) * 6 * (size_t)shells * g * g * words);
    trt_pointgrid G;
    trt_pointgrid_cone *cones = (trt_pointgrid_cone *)malloc(sizeof(trt_pointgrid_cone) * (size_t)(n ? n : 1));
    st->bits_set = (unsigned long long)trt_pointgrid_build(spheres, n, &cs, light, g, shells, &G, masks, cones);
    free(cones);
    st->cells = 6ull * shells * g * g;
    const double near = 0.02 + 4e-6 * sqrt((double)G.rg2);
    unsigned group_max = 0;
    for (size_t r = 0; r < n_rays; r++)
    {
        const double *o = rays + 6 * r, *d = o + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        int far;
        const int cell = trt_pointgrid_cell(&G, o[0], o[1], o[2], &far);
        st->rays++;
        if (far || !(fabs(a - 1.0) <= 9.094947017729282e-13))
        {
            st->far++;
            continue;
        }
        if (cell < 0 || cell >= 6 * shells * g * g)
        {
            note(st, o, -1, cell);
            continue;
        }
        const unsigned long long *m = masks + (size_t)cell * words;
        const double to_light[3] = {light[0] - o[0], light[1] - o[1], light[2] - o[2]};
        const double light_d2 = to_light[0] * to_light[0] + to_light[1] * to_light[1] + to_light[2] * to_light[2];
        const double light_d = sqrt(light_d2);
        unsigned cand = 0;
        for (int i = 0; i < n; i++)
        {
            double t;
            const int hit = exact_hit(o, d, a, spheres + 9 * i, &t);
            st->exact_hits += hit;
            cand += in_cell(m, i);
            if (hit && !in_cell(m, i) && t <= light_d + 0.5 * near)
                note(st, o, i, cell);
        }
        if (decide_lit(spheres, n, NULL, o, d, a, light_d2) != decide_lit(spheres, n, m, o, d, a, light_d2))
            st->decision_mismatches++;
        tally(st, cand, &group_max, r, n_rays);
    }
    free(masks);
    free(table);
}

/* TRT.c:677-695 */
static int plane_hit(const double *ground, const double *o, const double *d, double *t_out)
{
    const double *gp = ground, *gn = ground + 3;
    const double denom = d[0] * gn[0] + d[1] * gn[1] + d[2] * gn[2];
    if (!(fabs(denom) > 0.00001))
        return 0;
    const double t = ((gp[0] - o[0]) * gn[0] + (gp[1] - o[1]) * gn[1] + (gp[2] - o[2]) * gn[2]) / denom;
    *t_out = t;
    return t > 0.00001;
}

/* the reference's decision (TRT.c:805-853, :936-946) over all spheres and the ground (NULL: none) */
static int reference_lit(const double *spheres, int n, const double *ground, const double *o, const double *d, double a, double light_d2)
{
    double best_d2 = INFINITY, best_t = 0.0;
    int best = -1;
    for (int i = 0; i <= n; i++)
    {
        double t;
        if (i < n ? !exact_hit(o, d, a, spheres + 9 * i, &t) : !(ground && plane_hit(ground, o, d, &t)))
            continue;
        const double p[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        const double d2 = (o[0] - p[0]) * (o[0] - p[0]) + (o[1] - p[1]) * (o[1] - p[1]) + (o[2] - p[2]) * (o[2] - p[2]);
        if (d2 < best_d2)
            best_d2 = d2, best = i, best_t = t;
    }
    if (best < 0)
        return 1;
    /* TRT.c:871-874: normalize_vector leaves vectors of length <= 1e-4 alone */
    const double p[3] = {o[0] + best_t * d[0], o[1] + best_t * d[1], o[2] + best_t * d[2]};
    double back[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
    const double l = sqrt(back[0] * back[0] + back[1] * back[1] + back[2] * back[2]);
    if (l > 0.0001)
        back[0] /= l, back[1] /= l, back[2] /= l;
    double q[3];
    for (int k = 0; k < 3; k++)
        q[k] = (p[k] + back[k] * 0.000001) - o[k];
    return light_d2 < q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
}

typedef struct
{
    unsigned long long rays, far, dark, lit, unsure, wrong_dark, wrong_lit, tests, tests_closest;
    double first_wrong[6];
} anyhit_stats;

/* point_light_search of csrc/trt_rounds.hpp on the host: 0 dark, 1 lit, 2 unsure */
static int anyhit_class(const double *spheres, int n, const unsigned long long *m, const double *ground, const double *o, const double *d, double lo, double hi,
                        unsigned long long *tests)
{
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    int unsure = 0;
    for (int i = 0; i < n; i++)
    {
        if (!in_cell(m, i))
            continue;
        ++*tests;
        const double *s = spheres + 9 * i;
        const double ocx = o[0] - s[0], ocy = o[1] - s[1], ocz = o[2] - s[2];
        const double b = 2.0 * (ocx * d[0] + ocy * d[1] + ocz * d[2]);
        const double cc = (ocx * ocx + ocy * ocy + ocz * ocz) - s[3] * s[3];
        const double disc = b * b - 4.0 * a * cc;
        if (!(disc < 0.0) && b < 0.0)
        {
            const double q = -b - sqrt(disc), qq = q * q;
            const int blocks = q > TRT_SHADOW_QMIN && qq * TRT_SHADOW_K1 <= lo;
            if (blocks)
                return 0;
            unsure |= q > 0.0 && !(qq >= hi);
        }
    }
    if (ground)
    {
        const double *gp = ground, *gn = ground + 3;
        const double denom = d[0] * gn[0] + d[1] * gn[1] + d[2] * gn[2];
        if (fabs(denom) > 0.00001)
        {
            const double num = (gp[0] - o[0]) * gn[0] + (gp[1] - o[1]) * gn[1] + (gp[2] - o[2]) * gn[2];
            if (!((num < 0.0) != (denom < 0.0)) || num == 0.0) /* the kernel skips the division when the sign bits differ: t <= 0 then */
            {
                const double t = num / denom;
                if (t > 0.00001)
                {
                    const double qq = (t * t) * (4.0 * a) * a;
                    if (qq * TRT_SHADOW_K1 <= lo)
                        return 0;
                    unsure |= !(qq >= hi);
                }
            }
        }
    }
    return unsure ? 2 : 1;
}

void pointgrid_anyhit_check(const double *spheres, int n, const double *ground, const double *light, const double *rays, size_t n_rays, int g,
                            int shells, anyhit_stats *st)
{
    memset(st, 0, sizeof *st);
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    const int words = (n + 63) / 64 > 0 ? (n + 63) / 64 : 1;
    if (shells < 1)
        shells = 1;
    unsigned long long *masks = (unsigned long long *)malloc(sizeof(unsigned long long) * 6 * (size_t)shells * g * g * words);
    trt_pointgrid G;
    trt_pointgrid_cone *cones = (trt_pointgrid_cone *)malloc(sizeof(trt_pointgrid_cone) * (size_t)(n ? n : 1));
    trt_pointgrid_build(spheres, n, &cs, light, g, shells, &G, masks, cones);
    free(cones);
    for (size_t r = 0; r < n_rays; r++)
    {
        const double *o = rays + 6 * r, *d = o + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        int far;
        const int cell = trt_pointgrid_cell(&G, o[0], o[1], o[2], &far);
        st->rays++;
        if (far || !(fabs(a - 1.0) <= 9.094947017729282e-13) || cell < 0 || cell >= 6 * shells * g * g)
        {
            st->far++;
            continue;
        }
        const unsigned long long *m = masks + (size_t)cell * words;
        const double to_light[3] = {light[0] - o[0], light[1] - o[1], light[2] - o[2]};
        const double light_d2 = to_light[0] * to_light[0] + to_light[1] * to_light[1] + to_light[2] * to_light[2];
        double lo, hi;
        trt_point_shadow_bounds(&G, light_d2, a, &lo, &hi);
        const int cls = anyhit_class(spheres, n, m, ground, o, d, lo, hi, &st->tests);
        for (int i = 0; i < n; i++)
            st->tests_closest += (unsigned)in_cell(m, i);
        st->dark += cls == 0, st->lit += cls == 1, st->unsure += cls == 2;
        if (cls == 2)
            continue;
        const int ref = reference_lit(spheres, n, ground, o, d, a, light_d2);
        if (ref != cls)
        {
            if (!st->wrong_dark && !st->wrong_lit)
                memcpy(st->first_wrong, o, 6 * sizeof(double));
            st->wrong_dark += cls == 0, st->wrong_lit += cls == 1;
        }
    }
    free(masks);
    free(table);
}

/* The tables themselves, as the host reference builders make them (the GPU tests compare the device-built tables).
 * kind 0: directional light with to-light direction v, masks slabs*g*g*words; kind 1: point light at v, masks slabs*6*g*g*words
 * (`slabs` = slabs of depth resp. shells of distance, trt_lightgrid.h (5)). */
long lightgrid_host_table(const double *spheres, int n, int kind, const double *v, int g, int slabs, unsigned long long *masks)
{
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    free(table);
    long bits;
    if (kind == 0)
    {
        trt_dirgrid G;
        trt_dirgrid_disc *discs = (trt_dirgrid_disc *)malloc(sizeof(trt_dirgrid_disc) * (size_t)(n ? n : 1));
        bits = trt_dirgrid_build(spheres, n, &cs, v, g, slabs, &G, masks, discs);
        free(discs);
    }
    else
    {
        trt_pointgrid G;
        trt_pointgrid_cone *cones = (trt_pointgrid_cone *)malloc(sizeof(trt_pointgrid_cone) * (size_t)(n ? n : 1));
        bits = trt_pointgrid_build(spheres, n, &cs, v, g, slabs, &G, masks, cones);
        free(cones);
    }
    return bits;
}

/* ---- helpers of tests/test_candidate_edges.py ---- */

/* cell of the shadow ray that starts at o in the table of one light (kind and v as lightgrid_host_table), looked up as the kernel
 * does; -1 when the origin is outside the table's range */
long lightgrid_cell_of(const double *spheres, int n, int kind, const double *v, int g, int slabs, const double *o)
{
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    free(table);
    int far = 0;
    long cell;
    if (kind == 0)
    {
        trt_dirgrid G;
        trt_dirgrid_disc *discs = (trt_dirgrid_disc *)malloc(sizeof(trt_dirgrid_disc) * (size_t)(n ? n : 1));
        trt_dirgrid_prepare(spheres, n, &cs, v, g, slabs, &G, discs);
        free(discs);
        cell = trt_dirgrid_cell(&G, o[0], o[1], o[2], &far);
    }
    else
    {
        trt_pointgrid G;
        trt_pointgrid_cone *cones = (trt_pointgrid_cone *)malloc(sizeof(trt_pointgrid_cone) * (size_t)(n ? n : 1));
        trt_pointgrid_prepare(spheres, n, &cs, v, g, slabs, &G, cones);
        free(cones);
        cell = trt_pointgrid_cell(&G, o[0], o[1], o[2], &far);
    }
    return far ? -1 : cell;
}

/* the masks of a table packed into list cells with trt_list_pack, as the library packs them (csrc/trt_tables.hip: pack_cell): returns the
 * pool words used; a list that finds no room in `pool_cap` words leaves its cell TRT_LIST_NONE */
long lightgrid_pack(const unsigned long long *masks, long cells, int words, int bits, unsigned long long *lists, unsigned long long *pool, long pool_cap)
{
    long used = 0;
    for (long c = 0; c < cells; c++)
    {
        const unsigned long long *m = masks + c * words;
        const int count = trt_list_count(m, words);
        const long need = (long)trt_list_pool_words(count, bits);
        const int room = count <= 0xffff && used + need <= pool_cap;
        lists[c] = trt_list_pack(m, words, count, room ? pool : NULL, (unsigned)used, bits);
        if (room)
            used += need;
    }
    return used;
}

/* ---- helpers of tests/test_device_lookups.py: the host's own look-up of many origins at once, and the checks above on a cell the CALLER names ----
 * One light's table as the builders above make it: the same prepare, and per cell the same predicate the builders' loops evaluate -- a cell's
 * mask is formed when it is first asked for, so that a table of a million cells costs what the cells that are looked up cost. */

typedef struct
{
    int kind, n, g, depth, words; /* kind 0: directional light with to-light direction v, 1: point light at v */
    long cells;
    double v[3];
    trt_dirgrid D;
    trt_pointgrid P;
    trt_dirgrid_disc *discs;
    trt_pointgrid_cone *cones;
    unsigned long long *masks;
    unsigned char *have;
    unsigned long long border_bits; /* directional: bits set in the border cells the clamp relies on being empty */
} light_host;

static const unsigned long long *cell_mask(light_host *H, long cell)
{
    unsigned long long *m = H->masks + cell * H->words;
    if (H->have[cell])
        return m;
    const int g = H->g;
    for (int i = 0; i < H->n; i++)
    {
        int in;
        if (H->kind == 0) /* the body of trt_dirgrid_build's loop */
            in = trt_dirgrid_in_slab(H->discs + i, (int)(cell / ((long)g * g))) && trt_dirgrid_reaches(H->discs + i, (int)(cell % g), (int)((cell / g) % g));
        else /* of trt_pointgrid_build's */
            in = trt_pointgrid_in_shell(H->cones + i, (int)(cell / (6L * g * g)), H->P.shells) &&
                 trt_pointgrid_reaches(H->cones + i, (int)((cell / ((long)g * g)) % 6), (int)(cell % g), (int)((cell / g) % g), g);
        if (in)
            trt_lightgrid_set(m, i);
    }
    H->have[cell] = 1;
    return m;
}

light_host *light_host_build(const double *spheres, int n, int kind, const double *v, int g, int depth)
{
    light_host *H = (light_host *)calloc(1, sizeof *H);
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    free(table);
    if (depth < 1)
        depth = 1;
    H->kind = kind, H->n = n, H->g = g, H->depth = depth, H->words = (n + 63) / 64 > 0 ? (n + 63) / 64 : 1;
    H->cells = (long)depth * g * g * (kind ? 6 : 1);
    memcpy(H->v, v, sizeof H->v);
    H->discs = (trt_dirgrid_disc *)calloc((size_t)(n ? n : 1), sizeof(trt_dirgrid_disc));
    H->cones = (trt_pointgrid_cone *)calloc((size_t)(n ? n : 1), sizeof(trt_pointgrid_cone));
    if (kind == 0)
        trt_dirgrid_prepare(spheres, n, &cs, v, g, depth, &H->D, H->discs);
    else
        trt_pointgrid_prepare(spheres, n, &cs, v, g, depth, &H->P, H->cones);
    H->masks = (unsigned long long *)calloc((size_t)H->cells * H->words, sizeof(unsigned long long));
    H->have = (unsigned char *)calloc((size_t)H->cells, 1);
    if (kind == 0)
        for (int s = 0; s < depth; s++)
            for (int j = 0; j < g; j++)
                for (int c = 0; c < g; c++)
                    if (j == 0 || c == 0 || j == g - 1 || c == g - 1)
                    {
                        const unsigned long long *m = cell_mask(H, ((long)s * g + j) * g + c);
                        for (int w = 0; w < H->words; w++)
                            H->border_bits += (unsigned long long)__builtin_popcountll(m[w]);
                    }
    return H;
}

void light_host_free(light_host *H)
{
    free(H->discs), free(H->cones), free(H->masks), free(H->have);
    free(H);
}

/* the header as the host prepared it (the device stages its own copy): sizeof(trt_dirgrid) resp. sizeof(trt_pointgrid) bytes */
int light_host_header(const light_host *H, void *out)
{
    if (H->kind == 0)
        memcpy(out, &H->D, sizeof H->D);
    else
        memcpy(out, &H->P, sizeof H->P);
    return H->kind == 0 ? (int)sizeof H->D : (int)sizeof H->P;
}

/* normalize_vector of the reference (TRT.c:439-450): vectors not longer than 1e-4 are left alone */
static void ref_unit(const double v[3], double out[3])
{
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    out[0] = v[0], out[1] = v[1], out[2] = v[2];
    if (len > 0.0001)
        out[0] = v[0] / len, out[1] = v[1] / len, out[2] = v[2] / len;
}

/* the shadow ray the reference sends from o towards the light of H (TRT.c:903-907, :930-936) */
static void shadow_ray(const light_host *H, const double *o, double ray[6], double *light_d2)
{
    double to_light[3] = {H->v[0], H->v[1], H->v[2]};
    if (H->kind == 1)
        for (int k = 0; k < 3; k++)
            to_light[k] = H->v[k] - o[k];
    *light_d2 = to_light[0] * to_light[0] + to_light[1] * to_light[1] + to_light[2] * to_light[2];
    memcpy(ray, o, 3 * sizeof(double));
    ref_unit(to_light, ray + 3);
}

/* THE HOST'S OWN LOOK-UP of the shadow ray from every origin (3 doubles), as the shading stage performs it: far[r] (the grid's, or a direction
 * that is no unit vector), cell[r], and for a point light the bounds of the any-hit search; rays_out (6 doubles per origin, may be NULL): the
 * shadow ray itself */
void light_host_lookup(const light_host *H, const double *origins, size_t n_rays, int *far, int *cell, double *lo, double *hi, double *rays_out)
{
    for (size_t r = 0; r < n_rays; r++)
    {
        const double *o = origins + 3 * r;
        double ray[6], light_d2;
        shadow_ray(H, o, ray, &light_d2);
        const double a = ray[3] * ray[3] + ray[4] * ray[4] + ray[5] * ray[5];
        int f;
        if (H->kind == 0)
            cell[r] = trt_dirgrid_cell(&H->D, o[0], o[1], o[2], &f);
        else
        {
            cell[r] = trt_pointgrid_cell(&H->P, o[0], o[1], o[2], &f);
            f |= !(fabs(a - 1.0) <= 9.094947017729282e-13);
            trt_point_shadow_bounds(&H->P, light_d2, a, lo + r, hi + r);
        }
        far[r] = f;
        if (rays_out)
            memcpy(rays_out + 6 * r, ray, sizeof ray);
    }
}

/* dirgrid_check and pointgrid_check ON THE CALLER'S CELL: the shadow ray from origin r was looked up in cell[r] of the light's table (-1: not
 * looked up; counted as far).  Everything else is those two functions': a sphere the exact test hits must be in the cell -- for a point light
 * unless the hit is farther than the light + near / 2, rule (3) --, and the point light's lit / dark decision taken from the cell's spheres
 * must be the one taken from all spheres. */
void lightgrid_check_at(light_host *H, const double *spheres, const double *origins, const int *cell, size_t n_rays, grid_stats *st)
{
    memset(st, 0, sizeof *st);
    const int n = H->n;
    st->cells = (unsigned long long)H->cells;
    st->violations += 1000000ull * H->border_bits; /* the clamp relies on an empty border */
    const double near = 0.02 + 4e-6 * sqrt((double)H->P.rg2);
    unsigned group_max = 0;
    for (size_t r = 0; r < n_rays; r++)
    {
        double ray[6], light_d2;
        shadow_ray(H, origins + 3 * r, ray, &light_d2);
        const double *o = ray, *d = ray + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        st->rays++;
        if (cell[r] == -1 || !(fabs(a - 1.0) <= 9.094947017729282e-13))
        {
            st->far++;
            continue;
        }
        if (cell[r] < 0 || cell[r] >= H->cells)
        {
            note(st, o, -1, cell[r]);
            continue;
        }
        const unsigned long long *m = cell_mask(H, cell[r]);
        const double light_d = sqrt(light_d2);
        unsigned cand = 0;
        for (int i = 0; i < n; i++)
        {
            double t;
            const int hit = exact_hit(o, d, a, spheres + 9 * i, &t);
            st->exact_hits += hit;
            cand += in_cell(m, i);
            if (hit && !in_cell(m, i) && (H->kind == 0 || t <= light_d + 0.5 * near))
                note(st, o, i, cell[r]);
        }
        if (H->kind == 1 && decide_lit(spheres, n, NULL, o, d, a, light_d2) != decide_lit(spheres, n, m, o, d, a, light_d2))
            st->decision_mismatches++;
        tally(st, cand, &group_max, r, n_rays);
    }
}

/* pointgrid_anyhit_check on the caller's cell: what the any-hit search decides from the spheres of cell[r] must be the reference's answer */
void pointgrid_anyhit_check_at(light_host *H, const double *spheres, const double *ground, const double *origins, const int *cell, size_t n_rays,
                               anyhit_stats *st)
{
    memset(st, 0, sizeof *st);
    const int n = H->n;
    for (size_t r = 0; r < n_rays; r++)
    {
        double ray[6], light_d2;
        shadow_ray(H, origins + 3 * r, ray, &light_d2);
        const double *o = ray, *d = ray + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        st->rays++;
        if (H->kind != 1 || !(fabs(a - 1.0) <= 9.094947017729282e-13) || cell[r] < 0 || cell[r] >= H->cells)
        {
            st->far++;
            continue;
        }
        const unsigned long long *m = cell_mask(H, cell[r]);
        double lo, hi;
        trt_point_shadow_bounds(&H->P, light_d2, a, &lo, &hi);
        const int cls = anyhit_class(spheres, n, m, ground, o, d, lo, hi, &st->tests);
        for (int i = 0; i < n; i++)
            st->tests_closest += (unsigned)in_cell(m, i);
        st->dark += cls == 0, st->lit += cls == 1, st->unsure += cls == 2;
        if (cls == 2)
            continue;
        const int ref = reference_lit(spheres, n, ground, o, d, a, light_d2);
        if (ref != cls)
        {
            if (!st->wrong_dark && !st->wrong_lit)
                memcpy(st->first_wrong, o, 6 * sizeof(double));
            st->wrong_dark += cls == 0, st->wrong_lit += cls == 1;
        }
    }
}

/* do the list cells somebody else read at cell[r] (the device: words[r], long lists in `pool`, `bits` per entry) list exactly the spheres of the
 * host's mask of that cell, in ascending order?  Returns how many differ; cell -1: skipped */
long light_host_same_entries(light_host *H, const int *cell, const unsigned long long *words, const unsigned long long *pool, long pool_words, int bits,
                             size_t n_rays)
{
    long differ = 0;
    for (size_t r = 0; r < n_rays; r++)
    {
        if (cell[r] == -1)
            continue;
        if (cell[r] < 0 || cell[r] >= H->cells)
        {
            differ++;
            continue;
        }
        const unsigned long long *m = cell_mask(H, cell[r]);
        const int count = trt_list_count(m, H->words), e = trt_list_entries(words[r]);
        int same = e == count;
        if (same && ((unsigned)(words[r] >> 56) & TRT_LIST_POOLED) && (long)(unsigned)words[r] + (long)trt_list_pool_words(e, bits) > pool_words)
            same = 0;
        int k = 0;
        for (int i = 0; same && i < H->n; i++)
            if (in_cell(m, i))
                same = trt_list_entry(words[r], pool, k++, bits) == i;
        differ += !same;
    }
    return differ;
}

/* the FP32 filter (csrc/trt_filter.h) of many rays as the HOST evaluates it, for comparison with the device's (trt_selftest_filter): the nine
 * members of trt_ray_filter as 32-bit words per ray, the sign word of every sphere of the culling table (sphere-major: sign[sphere * n_rays + r])
 * and, dir_light != NULL, the fixed-direction sign words with the table of the directional light of that direction (TRT.c:903-904: the rays
 * towards it run along the normalised negated direction), as the kernels' scene image forms it */
void filter_host_words(const double *spheres, int n, const double *rays, size_t n_rays, const double *dir_light, unsigned *fields, unsigned *sign,
                       unsigned *sign_fixed)
{
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    float *kk_fixed = (float *)malloc(sizeof(float) * (size_t)(n ? n : 1));
    if (dir_light)
    {
        const double neg[3] = {dir_light[0] * -1.0, dir_light[1] * -1.0, dir_light[2] * -1.0};
        double tl[3];
        ref_unit(neg, tl);
        for (int i = 0; i < n; i++)
            kk_fixed[i] = trt_filter_fixed_dir_kk(table[4 * i], table[4 * i + 1], table[4 * i + 2], table[4 * i + 3], (float)tl[0], (float)tl[1], (float)tl[2]);
    }
    for (size_t r = 0; r < n_rays; r++)
    {
        const double *o = rays + 6 * r, *d = o + 3;
        trt_ray_filter f;
        trt_filter_setup(&f, o[0], o[1], o[2], d[0], d[1], d[2], d[0] * d[0] + d[1] * d[1] + d[2] * d[2], cs.c0[0], cs.c0[1], cs.c0[2], cs.cn, cs.rm);
        const float members[8] = {f.dx, f.dy, f.dz, f.wx, f.wy, f.wz, f.neg_thr, f.cd_min};
        memcpy(fields + 9 * r, members, sizeof members);
        fields[9 * r + 8] = (unsigned)f.ok;
        for (int i = 0; i < n; i++)
        {
            sign[(size_t)i * n_rays + r] = trt_filter_sign(&f, table[4 * i], table[4 * i + 1], table[4 * i + 2], table[4 * i + 3]);
            if (dir_light)
                sign_fixed[(size_t)i * n_rays + r] = trt_filter_sign_fixed_dir(&f, table[4 * i], table[4 * i + 1], table[4 * i + 2], kk_fixed[i]);
        }
    }
    free(kk_fixed);
    free(table);
}

/* centre (3) and admissible squared distance of a light's look-up: g0 and rg2 of a directional light's header, l and rg2 of a point light's */
void light_host_range(const light_host *H, double out[4])
{
    const double *c = H->kind == 0 ? H->D.g0 : H->P.l;
    out[0] = c[0], out[1] = c[1], out[2] = c[2], out[3] = (double)(H->kind == 0 ? H->D.rg2 : H->P.rg2);
}

/* (depth coordinate, face, row, column) of a cell index of the light's table (face 0 for a directional light) */
void light_host_coords(const light_host *H, const int *cell, size_t count, int *out)
{
    const long g = H->g;
    for (size_t r = 0; r < count; r++)
    {
        const long c = cell[r];
        const long plane = c / (g * g);
        out[4 * r] = (int)(H->kind ? plane / 6 : plane), out[4 * r + 1] = (int)(H->kind ? plane % 6 : 0);
        out[4 * r + 2] = (int)((c / g) % g), out[4 * r + 3] = (int)(c % g);
    }
}
