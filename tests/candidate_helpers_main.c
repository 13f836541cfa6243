/* The look-up, membership, prefilter and packing helpers tests/test_candidate_edges.py calls in raygrid_check.c and lightgrid_check.c,
 * run as a program of their own on a directed scene: a row of spheres along one direction from the eye and a ring of spheres off
 * that line, at 8- and 16-bit entry widths.  tests/test_candidate_edges.py compiles this with the two checkers under the address and
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
    free(sph), free(list);
    return bad;
}

int main(void)
{
    const int bad = run(20, 13) + run(300, 17);
    printf(bad ? "FAILED\n" : "ok\n");
    return bad != 0;
}
