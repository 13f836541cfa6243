/* The look-up, membership, prefilter and packing helpers tests/test_candidate_edges.py calls in raygrid_check.c and lightgrid_check.c,
 * run as a program of their own on a directed scene: a row of spheres along one direction from the eye and a ring of spheres off
 * that line, at 8- and 16-bit entry widths; on the same scenes the helpers of tests/test_device_lookups.py (the host's look-up of many rays, the checks
 * on a place the caller names).  tests/test_candidate_edges.py compiles this with the checkers (lean_lists_check.c holds raygrid_check.c) under the address and
 * undefined-behaviour sanitizers and runs it; it prints what it found and returns 0 when the figures are the directed ones. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

long raygrid_host_cells(const double *spheres, int n, const double *ground, const double *eye, int g_eye, int g_sph, int patch_m,
                        unsigned long long *cells, unsigned long long *pool, long pool_cap);
int raygrid_cell_of(const double *d, int g);
int raygrid_patch_of(int m, const double *w);
int raygrid_member(const double *spheres, int n, const double *ground, const double *eye, int patch_m, int table, const double *ray);
int raygrid_filter_survivors(const double *spheres, int n, const double *ray, const int *list, int count, int fixed_dir);
long lightgrid_host_table(const double *spheres, int n, int kind, const double *v, int g, int slabs, unsigned long long *masks);
long lightgrid_cell_of(const double *spheres, int n, int kind, const double *v, int g, int slabs, const double *o);
long lightgrid_pack(const unsigned long long *masks, long cells, int words, int bits, unsigned long long *lists, unsigned long long *pool, long pool_cap);

/* the helpers of tests/test_device_lookups.py (lean_lists_check.c, lightgrid_check.c): the host's own look-up of many rays, and the checks on a
 * place the caller names -- here the host's own */
typedef struct
{
    unsigned long long rays, judged, no_place, strangers, no_list, exact_hits, candidates, violations, lean_reads, lean_misses_own, full_hits_own;
    double first_violation[8];
} judged_stats;
typedef struct
{
    unsigned long long rays, far, exact_hits, candidates, violations, decision_mismatches, bits_set, cells, wave_max_cand, wave_groups, cand_hist[17];
    double first_violation[8];
} grid_stats;
typedef struct
{
    unsigned long long rays, far, dark, lit, unsure, wrong_dark, wrong_lit, tests, tests_closest;
    double first_wrong[6];
} anyhit_stats;
void *lookup_host_build(const double *spheres, int n, const double *ground, const double *eyes, int n_eyes, int g_eye, int g_sph, int patch_m);
void lookup_host_free(void *H);
void lookup_host_info(const void *H, long out[4]);
void lookup_path_host(const void *H, const double *spheres, const double *rays, const int *codes, const int *frames, size_t n_rays, int *out,
                      unsigned long long *words);
void lookup_path_members(const void *H, const double *rays, const int *region, const int *table, size_t n_rays, int *member);
void lookup_path_judge(const void *H, const double *spheres, const double *rays, const int *region, const int *table, const int *cell, size_t n_rays,
                       judged_stats *st);
int lookup_family_record(const void *H, int region, int table, double out[6]);
void lookup_cubemap_cells(const double *w, size_t count, int g, int *cell);
void lookup_along(const double *spheres, const double *rays, const int *own, size_t n_rays, double *out);
void *light_host_build(const double *spheres, int n, int kind, const double *v, int g, int depth);
void light_host_free(void *H);
void light_host_lookup(const void *H, const double *origins, size_t n_rays, int *far, int *cell, double *lo, double *hi, double *rays_out);
void lightgrid_check_at(void *H, const double *spheres, const double *origins, const int *cell, size_t n_rays, grid_stats *st);
void pointgrid_anyhit_check_at(void *H, const double *spheres, const double *ground, const double *origins, const int *cell, size_t n_rays, anyhit_stats *st);
long light_host_same_entries(void *H, const int *cell, const unsigned long long *words, const unsigned long long *pool, long pool_words, int bits, size_t n_rays);
void light_host_range(const void *H, double out[4]);
void light_host_coords(const void *H, const int *cell, size_t count, int *out);
void filter_host_words(const double *spheres, int n, const double *rays, size_t n_rays, const double *dir_light, unsigned *fields, unsigned *sign,
                       unsigned *sign_fixed);

static double unit_noise(unsigned long long *s)
{
    *s = *s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(long long)(*s >> 11) * 0x1p-52 - 1.0;
}

#define LOOKUP_RAYS 600
static int run_lookups(const double *sph, int n, const double *ground, int m)
{
    const double eyes[6] = {0.0, 1.0, -20.0, 3.0, 2.0, -18.0};
    int bad = 0;
    void *H = lookup_host_build(sph, n, ground, eyes, 2, 8, 4, m);
    if (!H)
        return 1;
    long info[4];
    lookup_host_info(H, info);
    static double rays[6 * LOOKUP_RAYS], out_along[LOOKUP_RAYS];
    static int codes[LOOKUP_RAYS], frames[LOOKUP_RAYS], out[8 * LOOKUP_RAYS], region[LOOKUP_RAYS], table[LOOKUP_RAYS], cell[LOOKUP_RAYS], member[LOOKUP_RAYS],
        own[LOOKUP_RAYS];
    static unsigned long long words[LOOKUP_RAYS];
    unsigned long long s = 77;
    for (int r = 0; r < LOOKUP_RAYS; r++)
    { /* from an eye, from a sphere's surface, and with codes that name nothing; a NaN among the directions */
        const int i = r % n, kind = r % 5;
        double d[3] = {unit_noise(&s), unit_noise(&s), unit_noise(&s)};
        const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        for (int k = 0; k < 3; k++)
            d[k] /= len, rays[6 * r + 3 + k] = d[k];
        frames[r] = r & 1;
        own[r] = kind == 1 ? i : -1;
        for (int k = 0; k < 3; k++)
            rays[6 * r + k] = kind == 1 ? sph[9 * i + k] + sph[9 * i + 3] * (1.0 + 1e-6) * d[k] : eyes[3 * frames[r] + k];
        codes[r] = kind == 0 ? 0 : kind == 1 ? 2 + i : kind == 2 ? 1 : kind == 3 ? -1 : 1000000 + r;
        if (r == 17)
            rays[6 * r + 4] = NAN;
    }
    lookup_path_host(H, sph, rays, codes, frames, LOOKUP_RAYS, out, words);
    long members = 0;
    for (int r = 0; r < LOOKUP_RAYS; r++)
    {
        const int is_member = out[8 * r + 3];
        region[r] = is_member ? out[8 * r] : -1, table[r] = out[8 * r + 1], cell[r] = out[8 * r + 2];
        members += is_member;
    }
    judged_stats st;
    lookup_path_judge(H, sph, rays, region, table, cell, LOOKUP_RAYS, &st);
    lookup_path_members(H, rays, region, table, LOOKUP_RAYS, member);
    for (int r = 0; r < LOOKUP_RAYS; r++)
        bad += region[r] >= 0 && !member[r];
    double rec[6];
    bad += lookup_family_record(H, 0, 3, rec) != 1 || lookup_family_record(H, 0, 4, rec) != 0 || lookup_family_record(H, 1, 2 * n * (m ? 6 * m * m : 1), rec) != 0;
    lookup_cubemap_cells(rays + 3, 1, 8, cell);
    lookup_along(sph, rays, own, LOOKUP_RAYS, out_along);
    printf("n %d patches %d: %ld cells (%ld without a list), %ld of %d rays are members, judged %llu, exact hits %llu, violations %llu, strangers %llu\n", n, m,
           info[0], info[1], members, LOOKUP_RAYS, st.judged, st.exact_hits, st.violations, st.strangers);
    bad += info[1] != 0 || members < LOOKUP_RAYS / 5 || st.violations || st.strangers || st.no_place || st.judged != (unsigned long long)members;
    lookup_host_free(H);
    /* the lights: the look-up of origins in and out of range, the checks on the host's own cells, the packed words of those cells */
    for (int kind = 0; kind < 2; kind++)
    {
        const double to_light[3] = {-0.3, 1.0, -0.2}, light[3] = {0.0, 30.0, 0.0};
        void *G = light_host_build(sph, n, kind, kind ? light : to_light, 8, 3);
        static double origins[3 * LOOKUP_RAYS], lo[LOOKUP_RAYS], hi[LOOKUP_RAYS], shadow[6 * LOOKUP_RAYS];
        static int far[LOOKUP_RAYS], coords[4 * LOOKUP_RAYS];
        for (int r = 0; r < LOOKUP_RAYS; r++)
            for (int k = 0; k < 3; k++)
                origins[3 * r + k] = (r % 7 == 6 ? 1e7 : 25.0) * unit_noise(&s) + (k == 2 ? 10.0 : 0.0);
        origins[5] = NAN, origins[6] = light[0], origins[7] = light[1], origins[8] = light[2];
        light_host_lookup(G, origins, LOOKUP_RAYS, far, cell, lo, hi, shadow);
        long near = 0;
        for (int r = 0; r < LOOKUP_RAYS; r++)
            cell[r] = far[r] ? -1 : cell[r], near += !far[r];
        grid_stats gs;
        anyhit_stats as;
        lightgrid_check_at(G, sph, origins, cell, LOOKUP_RAYS, &gs);
        pointgrid_anyhit_check_at(G, sph, ground, origins, cell, LOOKUP_RAYS, &as);
        double range[4];
        light_host_range(G, range);
        for (int r = 0; r < LOOKUP_RAYS; r++)
            region[r] = cell[r] < 0 ? 0 : cell[r];
        light_host_coords(G, region, LOOKUP_RAYS, coords);
        for (int r = 0; r < LOOKUP_RAYS; r++)
            words[r] = 0; /* an empty list: equal to the host's mask only where that is empty */
        const long differ = light_host_same_entries(G, cell, words, words, 0, 8, LOOKUP_RAYS);
        printf("n %d light kind %d: %ld of %d origins looked up, violations %llu, decision mismatches %llu, wrong %llu, %ld cells list something\n", n, kind, near,
               LOOKUP_RAYS, gs.violations, gs.decision_mismatches, as.wrong_dark + as.wrong_lit, differ);
        bad += near < LOOKUP_RAYS / 2 || far[1] != 1 || far[2] != kind || gs.violations || gs.decision_mismatches || as.wrong_dark || as.wrong_lit || differ < 0 || differ > near;
        light_host_free(G);
    }
    {
        static unsigned fields[9 * LOOKUP_RAYS];
        unsigned *sign = (unsigned *)malloc(sizeof(unsigned) * (size_t)n * LOOKUP_RAYS), *fixed = (unsigned *)malloc(sizeof(unsigned) * (size_t)n * LOOKUP_RAYS);
        const double dir[3] = {0.3, -1.0, 0.2};
        filter_host_words(sph, n, rays, LOOKUP_RAYS, dir, fields, sign, fixed);
        filter_host_words(sph, n, rays, LOOKUP_RAYS, NULL, fields, sign, NULL);
        bad += fields[9 * 17 + 8] != 0 || fields[8] != 1; /* the ray with a NaN is not ok */
        free(sign), free(fixed);
    }
    return bad;
}

static int run(int n, int row)
{
    const double eye[3] = {0.0, 1.0, -20.0}, ground[6] = {0.0, -2.0, 0.0, 0.0, 1.0, 0.0};
    const double len = sqrt(0.25 * 0.25 * 2 + 1.0), d[3] = {-0.25 / len, 0.25 / len, 1.0 / len};
    double *sph = (double *)calloc((size_t)n * 9, sizeof(double));
    int *list = (int *)malloc(sizeof(int) * (size_t)n);
    for (int i = 0; i < n; i++)
    {
        double *s = sph + 9 * i;
        if (i < row) /* on the line */
            for (int k = 0; k < 3; k++)
                s[k] = eye[k] + d[k] * (12.0 + 1.5 * i);
        else /* a wall behind the eye */
            s[0] = 1.2 * (i % 18) - 10.0, s[1] = 1.2 * (i / 18) + 3.0, s[2] = -60.0;
        s[3] = 0.25, s[4] = s[5] = s[6] = 0.5, s[7] = 0.3, s[8] = 100.0;
        list[i] = i;
    }
    int bad = 0;
    double ray[6] = {eye[0], eye[1], eye[2], d[0], d[1], d[2]};
    const int cell = raygrid_cell_of(d, 4);
    for (int m = 0; m <= 2; m++)
    {
        const int P = m ? 6 * m * m : 1, families = 2 + 2 * n * P;
        const int in_eye = raygrid_member(sph, n, ground, eye, m, 0, ray), in_last = raygrid_member(sph, n, ground, eye, m, families - 1, ray);
        const int outside = raygrid_member(sph, n, ground, eye, m, families, ray);
        printf("n %d patches %d: cell %d, member of the eye's family %d, of the last family %d, of none %d\n", n, m, cell, in_eye, in_last, outside);
        const int patch = raygrid_patch_of(m, d);
        bad += in_eye != 1 || outside != 0 || cell < 0 || cell >= 6 * 16 || patch < 0 || patch >= P;
    }
    const int kept = raygrid_filter_survivors(sph, n, ray, list, n, 0), kept_fixed = raygrid_filter_survivors(sph, n, ray, list, n, 1);
    printf("n %d: the filter keeps %d of %d (fixed direction: %d), %d on the line\n", n, kept, n, kept_fixed, row);
    bad += kept != row || kept_fixed != row;
    for (int kind = 0; kind < 2; kind++)
    {
        const int g = kind ? 2 : 8, words = (n + 63) / 64, bits = n > 256 ? 16 : 8;
        const long cells = kind ? 6 * g * g : g * g;
        const double to_light[3] = {-0.3, 1.0, -0.2}, light[3] = {0.0, 30.0, 0.0}, o[3] = {eye[0] + d[0] * 12.0, -1.95, eye[2] + d[2] * 12.0};
        const double *v = kind ? light : to_light;
        unsigned long long *masks = (unsigned long long *)calloc((size_t)(cells * words), 8), *lists = (unsigned long long *)calloc((size_t)cells, 8);
        const long cap = cells * 4;
        unsigned long long *pool = (unsigned long long *)calloc((size_t)cap, 8);
        lightgrid_host_table(sph, n, kind, v, g, 1, masks);
        const long used = lightgrid_pack(masks, cells, words, bits, lists, pool, cap), at = lightgrid_cell_of(sph, n, kind, v, g, 1, o);
        const long none = lightgrid_pack(masks, cells, words, bits, lists, pool, 0); /* no pool: long lists find no room */
        printf("n %d light kind %d: %ld cells, %ld pool words, origin in cell %ld\n", n, kind, cells, used, at);
        bad += used < 0 || used > cap || none != 0 || at < -1 || at >= cells;
        free(masks), free(lists), free(pool);
    }
    {
        const long total = 2 * 6 * 16 + 2 * (long)n * 6 * 9, cap = 2 * total + 16;
        unsigned long long *cells = (unsigned long long *)calloc((size_t)total, 8), *pool = (unsigned long long *)calloc((size_t)cap, 8);
        const long used = raygrid_host_cells(sph, n, ground, eye, 4, 3, 0, cells, pool, cap);
        const unsigned ctl = (unsigned)(cells[cell] >> 56);
        const int count = ctl & 0x80 ? (int)((cells[cell] >> 32) & 0xffff) : (int)ctl;
        printf("n %d: the eye's cell %d lists %d spheres (%ld pool words in all)\n", n, cell, count, used);
        bad += used < 0 || used > cap || count != row;
        free(cells), free(pool);
    }
    bad += run_lookups(sph, n, ground, n > 256 ? 1 : 2);
    free(sph), free(list);
    return bad;
}

int main(void)
{
    const int bad = run(20, 13) + run(300, 17);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
