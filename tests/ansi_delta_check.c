/* ansi_delta_check.c -- csrc/trt_ansi_delta.h, the format of the delta text between two RGB8 frames and the arithmetic the device kernels
 * (csrc/trt_ansi_delta.hpp) place its records by, compiled for the host and held against the sequential emitter trt_emitter_delta_rgb8
 * (csrc/host/trt_emit.c), which does not use the header.  A program of its own: tests/test_ansi_delta_layout.py builds and runs it plain and
 * under -fsanitize=address,undefined.
 *
 * For every width 1..70 x rows 1..4, 160 x 48 and 480 x 280, and every pattern family below, the text is assembled the way the kernels go
 * about it -- a length per cell from its neighbourhood (trt_delta_record_bytes), a sum per tile of TRT_DELTA_TILE cells, the exclusive scan
 * of the tiles' sums in turns of TRT_DELTA_SCAN_BLOCK, the scan within the tile lane by lane, the records' bytes by index
 * (trt_delta_record_byte), tile by tile -- into a buffer with a count per byte: the text equals the emitter's to the byte and in length,
 * every byte below the length was stored exactly once and none at or behind it, the length is within trt_delta_bound (and equals it where
 * every cell changed and all neighbours differ), and the limits hold.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_delta.h"
#include "trt_host.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_random(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 40);
}

static int g_failures;
static long g_cases;
#define FAIL(...)                                              \
    do                                                         \
    {                                                          \
        if (g_failures++ < 20)                                 \
        {                                                      \
            fprintf(stderr, "ansi_delta_check: " __VA_ARGS__); \
            fputc('\n', stderr);                               \
        }                                                      \
    } while (0)

enum
{
    NOTHING,       /* nothing changed */
    ALL_DIFFERENT, /* everything changed, all horizontal neighbours different: the bound */
    ALL_ONE,       /* everything changed, one colour */
    ALTERNATE,     /* every other cell */
    FIRST_ONLY,
    LAST_ONLY,
    ACROSS_ROWS,   /* a run into a row's last cell, one from the next row's first cell, the same colour */
    LEFT_COLOUR,   /* a changed cell whose new colour is its unchanged left neighbour's */
    RANDOM_TWO_001, RANDOM_TWO_40, RANDOM_TWO_99, RANDOM_FULL_001, RANDOM_FULL_40, RANDOM_FULL_99,
    FAMILIES
};
static const char *const k_family[FAMILIES] = {"nothing", "all different", "all one colour", "alternate", "first only", "last only", "across rows", "left colour",
                                               "random two 0.01", "random two 0.4", "random two 0.99", "random full 0.01", "random full 0.4", "random full 0.99"};

static void put(unsigned char *frame, long long p, unsigned rgb)
{
    frame[3 * p] = (unsigned char)rgb, frame[3 * p + 1] = (unsigned char)(rgb >> 8), frame[3 * p + 2] = (unsigned char)(rgb >> 16);
}
static unsigned get(const unsigned char *frame, long long p) { return (unsigned)frame[3 * p] | (unsigned)frame[3 * p + 1] << 8 | (unsigned)frame[3 * p + 2] << 16; }

/* a colour that is neither `a` nor `b` */
static unsigned other_than(unsigned a, unsigned b)
{
    unsigned c;
    do
        c = next_random() & 0xffffffu;
    while (c == a || c == b);
    return c;
}

static void make_frames(int family, int width, int rows, unsigned char *shown, unsigned char *next)
{
    const long long cells = (long long)width * rows;
    for (long long p = 0; p < cells; p++)
        put(shown, p, next_random() & 0xffffffu);
    memcpy(next, shown, (size_t)cells * 3);
    switch (family)
    {
    case NOTHING:
        break;
    case ALL_DIFFERENT:
        for (long long p = 0; p < cells; p++)
            put(next, p, other_than(get(shown, p), p % width ? get(next, p - 1) : get(shown, p)));
        break;
    case ALL_ONE:
        for (long long p = 0; p < cells; p++)
            put(shown, p, 0x102030u + (unsigned)(p & 1)), put(next, p, 0xa0b0c0u);
        break;
    case ALTERNATE:
        for (long long p = 0; p < cells; p += 2)
            put(next, p, other_than(get(shown, p), get(shown, p)));
        break;
    case FIRST_ONLY:
        put(next, 0, other_than(get(shown, 0), get(shown, 0)));
        break;
    case LAST_ONLY:
        put(next, cells - 1, other_than(get(shown, cells - 1), get(shown, cells - 1)));
        break;
    case ACROSS_ROWS:
        for (int r = 0; r + 1 < rows || r == 0; r++)
        { /* the last two cells of row r (where there are two) and the first two of row r + 1 */
            for (int c = width > 1 ? width - 2 : 0; c < width; c++)
                put(shown, (long long)r * width + c, 0x010101u), put(next, (long long)r * width + c, 0x00ff7fu);
            if (r + 1 < rows)
                for (int c = 0; c < 2 && c < width; c++)
                    put(shown, (long long)(r + 1) * width + c, 0x020202u), put(next, (long long)(r + 1) * width + c, 0x00ff7fu);
        }
        break;
    case LEFT_COLOUR:
        for (long long p = 1; p < cells; p += 3)
            if (get(shown, p) != get(shown, p - 1))
                put(next, p, get(next, p - 1));
        break;
    default:
    {
        const int two = family < RANDOM_FULL_001;
        const int which = (family - RANDOM_TWO_001) % 3;
        const unsigned threshold = which == 0 ? 167772u : which == 1 ? 6710886u : 16609443u; /* 0.01, 0.4, 0.99 of 2^24 */
        if (two)
            for (long long p = 0; p < cells; p++)
                put(shown, p, next_random() & 1 ? 0xffffffu : 0x000000u);
        memcpy(next, shown, (size_t)cells * 3);
        for (long long p = 0; p < cells; p++)
            if ((next_random() & 0xffffffu) < threshold)
                put(next, p, two ? get(shown, p) ^ 0xffffffu : other_than(get(shown, p), get(shown, p)));
        break;
    }
    }
}

/* what delta_cells of trt_ansi_delta.hpp gives a lane for cell p */
static trt_delta_flags flags_of(const unsigned char *shown, const unsigned char *next, int width, long long p)
{
    const int col = (int)(p % width);
    trt_delta_flags f;
    f.changed = get(shown, p) != get(next, p);
    f.changed_left = col > 0 && get(shown, p - 1) != get(next, p - 1);
    f.changed_right = col + 1 < width && get(shown, p + 1) != get(next, p + 1);
    f.same_as_left = p > 0 && get(next, p) == get(next, p - 1);
    return f;
}

static void check(int family, int width, int rows)
{
    const long long cells = (long long)width * rows;
    const unsigned long long bound = trt_delta_bound(width, rows), tiles = trt_delta_tiles((unsigned long long)cells);
    unsigned char *shown = (unsigned char *)malloc((size_t)cells * 3), *next = (unsigned char *)malloc((size_t)cells * 3);
    char *want = (char *)malloc((size_t)bound);
    unsigned char *got = (unsigned char *)calloc((size_t)bound + 64, 1), *stores = (unsigned char *)calloc((size_t)bound + 64, 1);
    unsigned *tile_bytes = (unsigned *)calloc((size_t)tiles, sizeof *tile_bytes);
    unsigned long long *tile_at = (unsigned long long *)calloc((size_t)tiles, sizeof *tile_at);
    size_t want_bytes = 0;
    g_cases++;
    make_frames(family, width, rows, shown, next);
    if (bound != (unsigned long long)rows * (21ull * width + 18))
        FAIL("%d x %d: bound %llu", width, rows, bound);
    if (trt_emitter_delta_rgb8(shown, next, width, rows, want, (size_t)bound, &want_bytes) != TRT_HOST_OK)
        FAIL("%s %d x %d: the emitter refused", k_family[family], width, rows);
    if (bound > 0 && trt_emitter_delta_rgb8(shown, next, width, rows, want, (size_t)bound - 1, &want_bytes) != TRT_HOST_ERR_ARGUMENT)
        FAIL("%d x %d: the emitter took a capacity below the bound", width, rows);
    /* measure: a sum per tile */
    for (unsigned long long t = 0; t < tiles; t++)
        for (long long p = (long long)t * TRT_DELTA_TILE; p < (long long)(t + 1) * TRT_DELTA_TILE && p < cells; p++)
        {
            const trt_delta_flags f = flags_of(shown, next, width, p);
            const unsigned n = trt_delta_record_bytes(&f);
            if (n != 0 && n != 2 && n != 6 && n != 21 && n != 25 && n != 35 && n != 39)
                FAIL("%s %d x %d: a record of %u bytes at cell %lld", k_family[family], width, rows, n, p);
            tile_bytes[t] += n;
        }
    /* offsets: turns of TRT_DELTA_SCAN_BLOCK sums, a running total */
    unsigned long long running = 0;
    for (unsigned long long first = 0; first < tiles; first += TRT_DELTA_SCAN_BLOCK)
    {
        unsigned long long turn = 0;
        for (unsigned long long t = first; t < first + TRT_DELTA_SCAN_BLOCK && t < tiles; t++)
            tile_at[t] = running + turn, turn += tile_bytes[t];
        running += turn;
    }
    const unsigned long long length = running;
    /* write: per tile, lane by lane, the lane's cells in order */
    for (unsigned long long t = 0; t < tiles; t++)
    {
        unsigned long long at = tile_at[t];
        for (int lane = 0; lane < TRT_DELTA_BLOCK; lane++)
            for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
            {
                const long long p = (long long)t * TRT_DELTA_TILE + (long long)lane * TRT_DELTA_LANE_CELLS + j;
                if (p >= cells)
                    continue;
                const trt_delta_flags f = flags_of(shown, next, width, p);
                const unsigned n = trt_delta_record_bytes(&f);
                for (unsigned k = 0; k < n; k++)
                {
                    if (at + k >= bound)
                    {
                        FAIL("%s %d x %d: a store behind the bound", k_family[family], width, rows);
                        break;
                    }
                    got[at + k] = (unsigned char)trt_delta_record_byte(k, (int)(p / width), (int)(p % width), get(next, p), &f);
                    stores[at + k]++;
                }
                at += n;
            }
    }
    if (length != want_bytes)
        FAIL("%s %d x %d: %llu bytes through the header, %zu from the emitter", k_family[family], width, rows, length, want_bytes);
    else if (memcmp(got, want, want_bytes) != 0)
    {
        size_t at = 0;
        while (got[at] == (unsigned char)want[at])
            at++;
        FAIL("%s %d x %d: the texts differ from byte %zu of %zu", k_family[family], width, rows, at, want_bytes);
    }
    for (unsigned long long i = 0; i < bound + 64; i++)
        if (stores[i] != (i < length ? 1 : 0))
        {
            FAIL("%s %d x %d: byte %llu of %llu stored %d times", k_family[family], width, rows, i, length, stores[i]);
            break;
        }
    if (length > bound)
        FAIL("%s %d x %d: %llu bytes, the bound is %llu", k_family[family], width, rows, length, bound);
    if (family == ALL_DIFFERENT && length != bound)
        FAIL("all different %d x %d: %llu bytes, the bound is %llu", width, rows, length, bound);
    if (family == NOTHING && length != 0)
        FAIL("nothing changed %d x %d: %llu bytes", width, rows, length);
    if (family == ALL_ONE && length != (unsigned long long)rows * (2ull * width + 14 + 19 + 4))
        FAIL("all one colour %d x %d: %llu bytes", width, rows, length);
    if (family == ACROSS_ROWS && rows > 1 && width >= 5 && length != 2ull * (rows - 1) * (14 + 19 + 2 * 2 + 4))
        FAIL("across rows %d x %d: %llu bytes: a cursor address and a colour per run, two runs of two cells per row boundary", width, rows, length);
    if (family == LEFT_COLOUR && width > 1)
    { /* every changed cell stands alone: a whole record of 39 bytes, colour included */
        unsigned long long changed = 0;
        for (long long p = 0; p < cells; p++)
            changed += get(shown, p) != get(next, p);
        if (length != 39 * changed)
            FAIL("left colour %d x %d: %llu bytes for %llu lone cells", width, rows, length, changed);
    }
    free(shown), free(next), free(want), free(got), free(stores), free(tile_bytes), free(tile_at);
}

int main(void)
{
    /* the limits and the bound */
    unsigned char px[6] = {0, 0, 0, 1, 1, 1};
    char text[64];
    size_t n = 0;
    if (!trt_delta_size_ok(TRT_DELTA_MAX_WIDTH, TRT_DELTA_MAX_ROWS) || trt_delta_size_ok(TRT_DELTA_MAX_WIDTH + 1, 1) || trt_delta_size_ok(1, TRT_DELTA_MAX_ROWS + 1) ||
        trt_delta_size_ok(0, 1) || trt_delta_size_ok(1, 0))
        FAIL("the limits");
    if (trt_delta_bound(TRT_DELTA_MAX_WIDTH + 1, 1) != 0 || trt_delta_bound(1, 0) != 0 || trt_delta_bound(TRT_DELTA_MAX_WIDTH, TRT_DELTA_MAX_ROWS) != 99999ull * (21ull * 49999 + 18))
        FAIL("the bound at the limits");
    if (TRT_DELTA_MAX_ROWS != 99999 || TRT_DELTA_MAX_WIDTH != 49999 || 2 * (TRT_DELTA_MAX_WIDTH - 1) + 1 > 99999 || TRT_DELTA_RECORD_MAX != 39)
        FAIL("the constants");
    if (trt_emitter_delta_rgb8(px, px + 3, 50000, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta_rgb8(px, px + 3, 1, 100000, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta_rgb8(px, px + 3, 0, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta_rgb8(NULL, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta_rgb8(px, px + 3, 1, 1, text, sizeof text, NULL) != TRT_HOST_ERR_ARGUMENT)
        FAIL("the emitter's refusals");
    /* the one cell, spelled out */
    if (trt_emitter_delta_rgb8(px, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_OK || n != 39 || memcmp(text, "\033[00001;00001H\033[48;2;001;001;001m  \033[0m", 39) != 0)
        FAIL("the record of a 1 x 1 screen");
    /* the last cell of the largest screen: five digits each */
    {
        const trt_delta_flags lone = {0, 1, 0, 0};
        char record[40] = {0};
        for (unsigned k = 0; k < trt_delta_record_bytes(&lone); k++)
            record[k] = (char)trt_delta_record_byte(k, TRT_DELTA_MAX_ROWS - 1, TRT_DELTA_MAX_WIDTH - 1, 0x0c22ffu, &lone);
        if (strcmp(record, "\033[99999;99997H\033[48;2;255;034;012m  \033[0m") != 0)
            FAIL("the record of the last cell of the largest screen");
    }
    for (int family = 0; family < FAMILIES; family++)
    {
        for (int width = 1; width <= 70; width++)
            for (int rows = 1; rows <= 4; rows++)
                check(family, width, rows);
        check(family, 160, 48);
        check(family, 480, 280);
    }
    if (g_failures)
    {
        fprintf(stderr, "ansi_delta_check: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("ansi_delta_check: ok (%ld cases)\n", g_cases);
    return 0;
}
