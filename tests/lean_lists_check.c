/* lean_lists_check.c -- host-side validation of the LEAN TWINS of the spheres' own families (csrc/trt_raygrid.h).
 * Test helper only: compiled by tests/test_lean_lists.py with gcc -O2 -ffp-contract=off -fopenmp.
 *
 * A path ray that starts on sphere i and leaves it outwards -- (o - c_i).d >= 0, the dot product the exact test forms --
 * reads its cell's list without entry i.  This file derives the twins with the header's own function (the one the device
 * kernel calls), compares twins cell by cell with "the full list minus the own sphere", and walks rays the way the kernel's
 * look-up does.  The tables, the family walk and the exact test are those of raygrid_check.c, included as they are. */
#include "raygrid_check.c"

typedef struct
{
    unsigned long long cells, stripped, unchanged, no_list, now_inline, still_pooled, copies, pool_words, violations;
    unsigned long long rays, own_members, lean_rays, lean_hits_own, negative_hits_own, candidates_full, candidates_lean, wave_max_full, wave_max_lean, wave_groups;
    double first_violation[8]; /* cell index, own, what | ray(6), sphere, what */
} lean_stats;

static void lean_note(lean_stats *st, double a, double b, double c)
{
    if (!st->violations)
        st->first_violation[0] = a, st->first_violation[1] = b, st->first_violation[2] = c;
    st->violations++;
}

/* Is `twin` the list of `full` without `own`: the same entries in the same (ascending) order, the same width, inline exactly
 * when they fit?  `may_copy`: a twin that found no room may be the full cell itself.  Returns 0 when it is. */
static int twin_differs(unsigned long long full, unsigned long long twin, const unsigned long long *pool, int own, int bits, int may_copy, lean_stats *st)
{
    const int e = trt_list_entries(full), inline_max = 56 / bits;
    int has_own = 0;
    for (int k = 0; k < e; k++)
        has_own |= trt_list_entry(full, pool, k, bits) == own;
    if (!has_own)
    { /* nothing to take out (or no list at all): the twin is the cell */
        st->unchanged++;
        st->no_list += e < 0;
        return twin != full;
    }
    if (twin == full && may_copy && e - 1 > inline_max)
    {
        st->copies++;
        return 0;
    }
    st->stripped++;
    const int t = trt_list_entries(twin);
    if (t != e - 1)
        return 1;
    const unsigned ctl = (unsigned)(twin >> 56);
    if (t <= inline_max ? ctl != (unsigned)t : ctl != TRT_LIST_POOLED)
        return 2;
    st->now_inline += t <= inline_max && e > inline_max;
    st->still_pooled += t > inline_max;
    int prev = -1;
    for (int k = 0, j = 0; k < e; k++)
    {
        const int i = trt_list_entry(full, pool, k, bits);
        if (i == own)
            continue;
        const int got = trt_list_entry(twin, pool, j++, bits);
        if (got != i || got <= prev)
            return 3;
        prev = got;
    }
    if (t <= inline_max && bits * t < 56 && ((twin & 0x00ffffffffffffffull) >> (bits * t)) != 0)
        return 4; /* unused inline entries are zero, as trt_list_pack leaves them */
    return 0;
}

/* Derive the twins of the n P non-mirrored tables `full` (P tables per sphere, table_cells cells each) as the device kernel
 * does -- trt_list_lean_words, then trt_list_lean with words taken from *pool_used on, up to pool_cap -- into `lean`, and
 * check every one of them.  `pool` holds the full tables' long lists and receives the twins'. */
void lean_derive(const unsigned long long *full, unsigned long long *lean, long cells, long table_cells, int P, unsigned long long *pool,
                 long *pool_used, long pool_cap, int bits, lean_stats *st)
{
    memset(st, 0, sizeof *st);
    st->cells = (unsigned long long)cells;
    for (long c = 0; c < cells; c++)
    {
        const int own = (int)(c / table_cells / P);
        const unsigned need = trt_list_lean_words(full[c], pool, own, bits);
        const int room = *pool_used + (long)need <= pool_cap;
        lean[c] = trt_list_lean(full[c], pool, own, bits, room, (unsigned)*pool_used);
        if (need && room)
            *pool_used += (long)need, st->pool_words += need;
        const int why = twin_differs(full[c], lean[c], pool, own, bits, !room, st);
        if (why)
            lean_note(st, (double)c, (double)own, (double)why);
    }
}

/* Twins somebody else derived (the device): the same check.  may_copy: the scene's part of the pool was capped. */
void lean_compare(const unsigned long long *full, const unsigned long long *lean, long cells, long table_cells, int P, const unsigned long long *pool,
                  int bits, int may_copy, lean_stats *st)
{
    memset(st, 0, sizeof *st);
    st->cells = (unsigned long long)cells;
    for (long c = 0; c < cells; c++)
    {
        const int own = (int)(c / table_cells / P);
        const int why = twin_differs(full[c], lean[c], pool, own, bits, may_copy, st);
        if (why)
            lean_note(st, (double)c, (double)own, (double)why);
    }
}

/* the host reference tables of a scene and their twins; returns the tables (lean_free) */
typedef struct
{
    tables *T;
    unsigned long long *lean; /* n P * 6 g_sph^2 */
    ray_stats build_stats;
} lean_tables;

lean_tables *lean_build(const double *spheres, int n, const double *ground, const double *eye, int g_eye, int g_sph, int patch_m, long pool_cap,
                        lean_stats *st)
{
    lean_tables *L = (lean_tables *)calloc(1, sizeof *L);
    L->T = build(spheres, n, ground, eye, g_eye, g_sph, patch_m, &L->build_stats);
    const long table_cells = 6L * g_sph * g_sph, cells = (long)n * L->T->patches.count * table_cells;
    L->lean = (unsigned long long *)malloc(sizeof(unsigned long long) * (size_t)(cells ? cells : 1));
    /* room for every twin unless the caller caps it: twins take at most the words their full lists took */
    const long cap = pool_cap >= 0 ? (long)L->T->pool_words + pool_cap : 2 * (long)L->T->pool_words + 16;
    L->T->pool = (unsigned long long *)realloc(L->T->pool, sizeof(unsigned long long) * (size_t)(cap > (long)L->T->pool_cap ? cap : (long)L->T->pool_cap));
    long used = (long)L->T->pool_words;
    lean_derive(L->T->cells + family_base(L->T, 2), L->lean, cells, table_cells, L->T->patches.count, L->T->pool, &used, cap, L->T->bits, st);
    return L;
}

void lean_free(lean_tables *L)
{
    destroy(L->T);
    free(L->lean);
    free(L);
}

/* dot(sub(o, c), d) in the kernel's operation order (csrc/trt_device.hpp): half the exact test's b, bit for bit */
static double along(const double *o, const double *c, const double *d)
{
    const double wx = o[0] - c[0], wy = o[1] - c[1], wz = o[2] - c[2];
    return wx * d[0] + wy * d[1] + wz * d[2];
}

/* One ray looked up as path_cell looks it up in table 2 + i P + k of sphere i: *out = the cell it reads (the twin iff the dot is
 * >= 0), returns -1 not a member, 0 the full cell, 1 the twin */
static int lean_lookup(const lean_tables *L, const double *spheres, int i, int k, const double *o, const double *d, unsigned long long *out)
{
    const tables *T = L->T;
    const int table = 2 + i * T->patches.count + k;
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!(fabs(a - 1.0) <= 9.094947017729282e-13) || !trt_rayfamily_member(&T->fam[table], o[0], o[1], o[2], d[0], d[1], d[2]))
        return -1;
    const int g = T->g_sph;
    const int c = trt_cubemap_cell((float)d[0], (float)d[1], (float)d[2], 0.5f * (float)g, (float)(g - 1), g);
    const int lean = along(o, spheres + 9 * i, d) >= 0.0;
    *out = lean ? L->lean[((size_t)i * T->patches.count + k) * 6 * (size_t)g * g + (size_t)c] : T->cells[family_base(T, table) + (size_t)c];
    return lean;
}

static void ray_note(lean_stats *st, const double *ray, int sphere, int what)
{
    if (!st->violations)
    {
        memcpy(st->first_violation, ray, 6 * sizeof(double));
        st->first_violation[6] = sphere, st->first_violation[7] = what;
    }
    st->violations++;
}

/* CONSERVATIVENESS.  rays: n_rays x 6 doubles, kinds[r] == 0 marks the rays to look at.  Every such ray is looked up in EVERY
 * non-mirrored family of a sphere it is a member of (all_families) or in the family of sphere own[r] alone (own != NULL; -1:
 * skip), on the patch its origin names.  A ray that reads the twin (dot >= 0) must miss its own sphere in the reference's test,
 * and every sphere the reference's test hits must be in the list the ray reads -- twin or full.  Rays with a negative dot that do
 * hit their own sphere are counted (negative_hits_own): they were answered from the full list, which holds it. */
void lean_rays_check(const lean_tables *L, const double *spheres, int n, const double *rays, const unsigned char *kinds, const int *own, size_t n_rays,
                     lean_stats *st)
{
    const tables *T = L->T;
    unsigned group_full = 0, group_lean = 0;
    size_t seen = 0;
    for (size_t r = 0; r < n_rays; r++)
    {
        if (kinds && kinds[r] != 0)
            continue;
        const double *o = rays + 6 * r, *d = o + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        st->rays++;
        for (int i = own ? own[r] : 0; i >= 0 && i < (own ? own[r] + 1 : n); i++)
        {
            const int k = trt_patch_of(T->patches.m, o[0] - spheres[9 * i], o[1] - spheres[9 * i + 1], o[2] - spheres[9 * i + 2]);
            unsigned long long cell = 0, full = 0;
            const int lean = lean_lookup(L, spheres, i, k, o, d, &cell);
            if (lean < 0 || lookup(T, 2 + i * T->patches.count + k, o, d, &full) < 0)
                continue; /* not a member, or a cell without a list: the wave sweeps */
            st->own_members++;
            st->lean_rays += (unsigned)lean;
            const unsigned cf = (unsigned)trt_list_entries(full), cl = (unsigned)trt_list_entries(cell);
            st->candidates_full += cf, st->candidates_lean += cl;
            group_full = cf > group_full ? cf : group_full, group_lean = cl > group_lean ? cl : group_lean;
            if ((++seen & 63) == 0)
                st->wave_max_full += group_full, st->wave_max_lean += group_lean, st->wave_groups++, group_full = group_lean = 0;
            for (int j = 0; j < n; j++)
            {
                double t;
                const int hit = exact_hit(o, d, a, spheres + 9 * j, &t);
                if (j == i && hit)
                {
                    st->lean_hits_own += lean;
                    st->negative_hits_own += !lean;
                    if (lean)
                        ray_note(st, o, j, 1); /* dot >= 0 and the reference hits the own sphere: the sign argument is broken */
                }
                if (hit && in_list(T, cell, j) != 1)
                    ray_note(st, o, j, 2); /* an exact hit that the list the ray reads does not hold */
            }
        }
    }
}

void lean_stats_clear(lean_stats *st) { memset(st, 0, sizeof *st); }

/* the full cells (non-mirrored tables only), the twins and the pool of a lean_tables, for comparisons in Python */
long lean_cells(const lean_tables *L, const unsigned long long **full, const unsigned long long **lean, const unsigned long long **pool, int *bits)
{
    const tables *T = L->T;
    *full = T->cells + family_base(T, 2), *lean = L->lean, *pool = T->pool, *bits = T->bits;
    return (long)T->n * T->patches.count * 6L * T->g_sph * T->g_sph;
}

/* one list cell's entries into out[cap]; returns the count (-1: no list) */
int lean_cell_entries(unsigned long long cell, const unsigned long long *pool, int bits, int *out, int cap)
{
    const int e = trt_list_entries(cell);
    for (int k = 0; k < e && k < cap; k++)
        out[k] = trt_list_entry(cell, pool, k, bits);
    return e;
}

/* do two sets of list cells hold the same entries cell by cell (their pool offsets may differ)?  returns the number that differ */
long lean_same_entries(const unsigned long long *a, const unsigned long long *a_pool, const unsigned long long *b, const unsigned long long *b_pool,
                       long cells, int bits)
{
    long differ = 0;
    for (long c = 0; c < cells; c++)
    {
        const int e = trt_list_entries(a[c]);
        int same = e == trt_list_entries(b[c]) && (a[c] >> 56) == (b[c] >> 56);
        for (int k = 0; same && k < e; k++)
            same = trt_list_entry(a[c], a_pool, k, bits) == trt_list_entry(b[c], b_pool, k, bits);
        differ += !same;
    }
    return differ;
}
