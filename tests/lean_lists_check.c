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

/* ---- helpers of tests/test_device_lookups.py: the host's own look-up of many rays at once, and the checks above on a place the CALLER names ----
 * A place is (region, table, cell): region 0 the eye's tables (table = 2 frame + family, frame < the number of eyes the host was built for),
 * 1 the 2 n P tables of the spheres (library order: patch k of sphere i at i P + k, then the mirror images), 2 the lean twins (n P); region -1:
 * not looked up.  The tables, the family records, the membership test, the exact test and the lean rule are those of the checks above. */

typedef struct
{
    lean_tables *L;  /* the families and tables of eye 0 and of the spheres, and the twins */
    int n_eyes;
    tables *eyes[8]; /* eyes 1..: the two families of that eye and their tables alone */
} lookup_host;

/* the two families of one eye and their tables, packed like build() packs them */
static tables *build_eye_only(const double *spheres, int n, const double *ground, const double *eye, int g_eye)
{
    tables *T = (tables *)calloc(1, sizeof *T);
    trt_patchset_init(&T->patches, 0);
    T->n = n, T->g_eye = g_eye, T->g_sph = 0, T->families = 2;
    T->fam = (trt_rayfamily *)malloc(sizeof(trt_rayfamily) * 2);
    const int padded = trt_cull_padded(n, 8);
    float *table = (float *)malloc(sizeof(float) * 4 * (size_t)(padded ? padded : 1));
    trt_cull_scene cs;
    trt_cull_build(spheres, n, 8, table, &cs);
    free(table);
    trt_eye_families(eye, ground, &cs, T->fam);
    const int words = (n + 63) / 64 > 0 ? (n + 63) / 64 : 1;
    const size_t cells = 6 * (size_t)g_eye * g_eye;
    T->bits = n > TRT_LIST_MAX_SPHERES ? 16 : 8;
    T->cells = (unsigned long long *)malloc(sizeof(unsigned long long) * 2 * cells);
    T->pool_cap = 2 * cells * (size_t)((n * T->bits + 63) / 64 + 1);
    T->pool = (unsigned long long *)malloc(sizeof(unsigned long long) * T->pool_cap);
    unsigned long long *masks = (unsigned long long *)malloc(sizeof(unsigned long long) * cells * words);
    trt_pointgrid_cone *cones = (trt_pointgrid_cone *)malloc(sizeof(trt_pointgrid_cone) * (size_t)(n ? n : 1));
    for (int f = 0; f < 2; f++)
    {
        trt_rayfamily_build(spheres, n, &T->fam[f], g_eye, masks, cones);
        for (size_t c = 0; c < cells; c++)
        {
            const int count = trt_list_count(masks + c * words, words);
            const size_t need = trt_list_pool_words(count, T->bits), at = T->pool_words;
            const int room = at + need <= T->pool_cap;
            if (room)
                T->pool_words += need;
            T->cells[f * cells + c] = trt_list_pack(masks + c * words, words, count, room ? T->pool : NULL, (unsigned)at, T->bits);
        }
    }
    free(cones);
    free(masks);
    return T;
}

lookup_host *lookup_host_build(const double *spheres, int n, const double *ground, const double *eyes, int n_eyes, int g_eye, int g_sph, int patch_m)
{
    if (n_eyes < 1 || n_eyes > 8)
        return NULL;
    lookup_host *H = (lookup_host *)calloc(1, sizeof *H);
    lean_stats st;
    g_pool_words_factor = 4; /* the judge needs every list: no cell may be left without one for want of pool words (lookup_host_info reports) */
    H->L = lean_build(spheres, n, ground, eyes, g_eye, g_sph, patch_m, -1, &st);
    g_pool_words_factor = 1;
    H->n_eyes = n_eyes;
    for (int b = 1; b < n_eyes; b++)
        H->eyes[b] = build_eye_only(spheres, n, ground, eyes + 3 * b, g_eye);
    if (st.violations)
    { /* the twins failed their own check: nothing to judge with */
        for (int b = 1; b < n_eyes; b++)
            destroy(H->eyes[b]);
        lean_free(H->L);
        free(H);
        return NULL;
    }
    return H;
}

/* cells of eye 0's and the spheres' tables, how many of them have no list, pool words used, pool words set aside */
void lookup_host_info(const lookup_host *H, long out[4])
{
    const ray_stats *b = &H->L->build_stats;
    out[0] = (long)b->cells, out[1] = (long)b->none_cells, out[2] = (long)b->pool_words, out[3] = (long)H->L->T->pool_cap;
}

void lookup_host_free(lookup_host *H)
{
    for (int b = 1; b < H->n_eyes; b++)
        destroy(H->eyes[b]);
    lean_free(H->L);
    free(H);
}

/* family record, list cell and pool of a place; 0 if there is no such place */
static int place_of(const lookup_host *H, int region, int table, int cell, const trt_rayfamily **fam, unsigned long long *word, const unsigned long long **pool)
{
    const tables *T = H->L->T;
    const int P = T->patches.count, n = T->n;
    const long ce = 6L * T->g_eye * T->g_eye, cs = 6L * T->g_sph * T->g_sph;
    if (region == 0)
    {
        const int frame = table >> 1, f = table & 1;
        if (table < 0 || frame >= H->n_eyes || cell < 0 || cell >= ce)
            return 0;
        const tables *E = frame ? H->eyes[frame] : T;
        *fam = &E->fam[f], *word = E->cells[(size_t)f * ce + cell], *pool = E->pool;
        return 1;
    }
    if (cell < 0 || cell >= cs || table < 0)
        return 0;
    if (region == 1 && table < 2 * n * P)
    {
        *fam = &T->fam[2 + table], *word = T->cells[family_base(T, 2 + table) + (size_t)cell], *pool = T->pool;
        return 1;
    }
    if (region == 2 && table < n * P)
    {
        *fam = &T->fam[2 + table], *word = H->L->lean[(size_t)table * cs + cell], *pool = T->pool;
        return 1;
    }
    return 0;
}

static int unit_member(const trt_rayfamily *F, const double *o, const double *d)
{
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    return fabs(a - 1.0) <= 9.094947017729282e-13 && trt_rayfamily_member(F, o[0], o[1], o[2], d[0], d[1], d[2]);
}

/* THE HOST'S OWN LOOK-UP of ray r with the kernel's family code codes[r] in frame frames[r] (NULL: 0), as path_cell / path_cell_patches are
 * specified: the table the code names (table_of), the cell of the direction, the twin where the ray leaves its own sphere outwards.
 * out[8 r ..]: region, table, cell (of the place the host reads if the ray is a member; -1s for a code that names no family), member (0 / 1),
 * successor code (of a reflection by the ground; with patches -- without, the code itself, which the look-up leaves alone), patch, face-major
 * cell coordinates are the caller's to derive; has_list (the cell is no TRT_LIST_NONE), lean (the dot is >= 0).  words[r]: the cell there. */
void lookup_path_host(const lookup_host *H, const double *spheres, const double *rays, const int *codes, const int *frames, size_t n_rays, int *out,
                      unsigned long long *words)
{
    const tables *T = H->L->T;
    const int n = T->n, P = T->patches.count, m = T->patches.m;
#pragma omp parallel for schedule(static)
    for (size_t r = 0; r < n_rays; r++)
    {
        const double *o = rays + 6 * r, *d = o + 3;
        int *q = out + 8 * r;
        const int code = codes[r], frame = frames ? frames[r] : 0;
        for (int k = 0; k < 8; k++)
            q[k] = -1;
        q[3] = q[6] = q[7] = 0;
        words[r] = 0;
        int valid = code == 0 || code == 1 || (code >= 2 && code < 2 + n);
        if (!valid && code >= 2 + n)
        {
            const int rest = code - 2 - n;
            valid = m ? ((rest >> TRT_PATCH_SHIFT) < n && (rest & ((1 << TRT_PATCH_SHIFT) - 1)) < P) : rest < n;
        }
        if (!valid || frame < 0 || frame >= H->n_eyes)
            continue;
        int patch = 0, region, table;
        const int fam_index = m || code < 2 + n ? table_of(T, spheres, code, o, &patch) : 2 + (n + (code - 2 - n)); /* without patches the mirror code is 2 + n + i */
        const int own = code >= 2 && code < 2 + n ? code - 2 : -1;
        const int lean = own >= 0 && along(o, spheres + 9 * own, d) >= 0.0;
        if (code < 2)
            region = 0, table = 2 * frame + code;
        else
            region = lean ? 2 : 1, table = fam_index - 2;
        const int g = code < 2 ? T->g_eye : T->g_sph;
        const int c = trt_cubemap_cell((float)d[0], (float)d[1], (float)d[2], 0.5f * (float)g, (float)(g - 1), g);
        const trt_rayfamily *F;
        unsigned long long word;
        const unsigned long long *pool;
        q[0] = region, q[1] = table, q[2] = c, q[5] = patch, q[7] = lean;
        q[4] = !m ? code : (code == 0 ? 1 : (own >= 0 ? 2 + n + ((own << TRT_PATCH_SHIFT) | patch) : -1));
        if (!place_of(H, region, table, c, &F, &word, &pool))
            continue; /* a direction without a cell (NaN): no member either */
        q[3] = unit_member(F, o, d);
        q[6] = (unsigned)(word >> 56) != TRT_LIST_NONE;
        words[r] = q[3] ? word : 0;
    }
}

/* is ray r a member (unit direction included) of the family of place (region[r], table[r])?  0 for a place that does not exist */
void lookup_path_members(const lookup_host *H, const double *rays, const int *region, const int *table, size_t n_rays, int *member)
{
#pragma omp parallel for schedule(static)
    for (size_t r = 0; r < n_rays; r++)
    {
        const trt_rayfamily *F;
        unsigned long long word;
        const unsigned long long *pool;
        member[r] = place_of(H, region[r], table[r], 0, &F, &word, &pool) && unit_member(F, rays + 6 * r, rays + 6 * r + 3);
    }
}

typedef struct
{
    unsigned long long rays, judged, no_place, strangers, no_list, exact_hits, candidates, violations, lean_reads, lean_misses_own, full_hits_own;
    double first_violation[8]; /* ray(6), sphere, what: 1 a twin was read and the own sphere is hit, 2 an exact hit the list does not hold, 3 a malformed list */
} judged_stats;

/* THE CONSERVATIVENESS CHECK ON THE CALLER'S PLACE: ray r was looked up at (region[r], table[r], cell[r]); region -1: not looked up, skipped.
 * The rules are raygrid_check's and lean_rays_check's: every sphere the reference's exact test hits must be in the list at that place; where the
 * place is a twin, its own sphere (table / P) may be missing only where its own test misses.  Counted beside the violations: places that do
 * not exist (no_place), rays that are no members of the family of the place they were looked up in (strangers: the tables promise them
 * nothing), places without a list (no_list: nothing to judge, the ray's wave sweeps). */
void lookup_path_judge(const lookup_host *H, const double *spheres, const double *rays, const int *region, const int *table, const int *cell, size_t n_rays,
                       judged_stats *st)
{
    const tables *T = H->L->T;
    const int n = T->n, P = T->patches.count;
    memset(st, 0, sizeof *st);
    for (size_t r = 0; r < n_rays; r++)
    {
        st->rays++;
        if (region[r] == -1)
            continue;
        const double *o = rays + 6 * r, *d = o + 3;
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        const trt_rayfamily *F;
        unsigned long long word;
        const unsigned long long *pool;
        if (!place_of(H, region[r], table[r], cell[r], &F, &word, &pool))
        {
            st->no_place++;
            continue;
        }
        if (!unit_member(F, o, d))
        {
            st->strangers++;
            continue;
        }
        if ((unsigned)(word >> 56) == TRT_LIST_NONE)
        {
            st->no_list++;
            continue;
        }
        st->judged++;
        const int own = region[r] == 2 ? table[r] / P : -1;
        st->lean_reads += own >= 0;
        const int e = trt_list_entries(word);
        st->candidates += (unsigned)e;
        int prev = -1, malformed = 0;
        unsigned char listed[TRT_PATH_MAX_SPHERES];
        memset(listed, 0, (size_t)n);
        for (int k = 0; k < e; k++)
        {
            const int i = trt_list_entry(word, pool, k, T->bits);
            malformed |= i <= prev || i >= n;
            if (i >= 0 && i < n)
                listed[i] = 1;
            prev = i;
        }
        if (malformed)
        {
            if (!st->violations)
            {
                memcpy(st->first_violation, o, 6 * sizeof(double));
                st->first_violation[6] = -1, st->first_violation[7] = 3;
            }
            st->violations++;
        }
        for (int j = 0; j < n && !malformed; j++)
        {
            double t;
            const int hit = exact_hit(o, d, a, spheres + 9 * j, &t);
            st->exact_hits += hit;
            const int in = listed[j];
            if (j == own)
                st->lean_misses_own += !hit;
            if (region[r] == 1 && table[r] < n * P && j == table[r] / P)
                st->full_hits_own += hit;
            if (hit && !in)
            {
                if (!st->violations)
                {
                    memcpy(st->first_violation, o, 6 * sizeof(double));
                    st->first_violation[6] = j, st->first_violation[7] = j == own ? 1 : 2;
                }
                st->violations++;
            }
        }
    }
}

/* do the list cells somebody else read (the device: words[r], long lists in `pool`) hold the entries of the host's cell at the place named,
 * in the same order and with the same control byte?  Returns how many differ (a place that does not exist differs). */
long lookup_path_same_entries(const lookup_host *H, const int *region, const int *table, const int *cell, const unsigned long long *words,
                              const unsigned long long *pool, long pool_words, size_t n_rays)
{
    const int bits = H->L->T->bits;
    long differ = 0;
    for (size_t r = 0; r < n_rays; r++)
    {
        if (region[r] == -1)
            continue;
        const trt_rayfamily *F;
        unsigned long long mine;
        const unsigned long long *my_pool;
        if (!place_of(H, region[r], table[r], cell[r], &F, &mine, &my_pool))
        {
            differ++;
            continue;
        }
        const int e = trt_list_entries(mine);
        int same = e == trt_list_entries(words[r]) && (mine >> 56) == (words[r] >> 56);
        if (same && ((unsigned)(words[r] >> 56) & TRT_LIST_POOLED) && e > 0 &&
            (long)(unsigned)words[r] + (long)trt_list_pool_words(e, bits) > pool_words)
            same = 0; /* a pooled list that ends outside the pool it was read with */
        for (int k = 0; same && k < e; k++)
            same = trt_list_entry(mine, my_pool, k, bits) == trt_list_entry(words[r], pool, k, bits);
        differ += !same;
    }
    return differ;
}

/* cube-map cell of many directions, and its (face, row, column): the look-up of path_cell's cells (w = the direction) and of the patches (w =
 * origin - centre, g = m), as the HOST evaluates it */
void lookup_cubemap_cells(const double *w, size_t count, int g, int *cell)
{
    for (size_t r = 0; r < count; r++)
        cell[r] = g ? trt_cubemap_cell((float)w[3 * r], (float)w[3 * r + 1], (float)w[3 * r + 2], 0.5f * (float)g, (float)(g - 1), g) : 0;
}

/* the family record of a place's table: apex (3), r_chk, r_chk^2, rg^2; returns 0 for a place that does not exist */
int lookup_family_record(const lookup_host *H, int region, int table, double out[6])
{
    const trt_rayfamily *F;
    unsigned long long word;
    const unsigned long long *pool;
    if (!place_of(H, region, table, 0, &F, &word, &pool))
        return 0;
    out[0] = F->a[0], out[1] = F->a[1], out[2] = F->a[2], out[3] = F->r_chk, out[4] = F->r_chk2, out[5] = F->rg2;
    return 1;
}

/* dot(o - c_i, d) of many rays, i = own[r] (-1: 0.0), as the exact test and the look-up form it: the sign that chooses the twin */
void lookup_along(const double *spheres, const double *rays, const int *own, size_t n_rays, double *out)
{
    for (size_t r = 0; r < n_rays; r++)
        out[r] = own[r] >= 0 ? along(rays + 6 * r, spheres + 9 * own[r], rays + 6 * r + 3) : 0.0;
}
