/* ansi_delta_half_check.c -- csrc/trt_ansi_delta_half.h, the format of the delta text between two RGB8 frames in half-block cells and the
 * arithmetic the device kernels (csrc/trt_ansi_delta_half.hpp) place its records by, compiled for the host and held against the sequential
 * emitter trt_emitter_delta_half_rgb8 (csrc/host/trt_emit.c), which does not use the header.  A program of its own:
 * tests/test_ansi_delta_half_layout.py builds and runs it plain and under -fsanitize=address,undefined.
 *
 * For every width 1..70 x rows 1..5 (odd and even frames, one text row), 160 x 47, 160 x 48 and 480 x 280, and every pattern family below,
 * the text is assembled the way the kernels go about it -- a length per cell from its neighbourhood (trt_delta_half_record_bytes), a sum per
 * tile of TRT_DELTA_TILE cells, the exclusive scan of the tiles' sums in turns of TRT_DELTA_SCAN_BLOCK, the scan within the tile lane by
 * lane, the records' bytes by index (trt_delta_half_record_byte), tile by tile -- into a buffer with a count per byte: the text equals the
 * emitter's to the byte and in length, every byte below the length was stored exactly once and none at or behind it, the length is within
 * trt_delta_half_bound (and equals it where every cell changed and both colours differ from the left neighbour's everywhere), and the
 * limits hold.  The frames are allocated at exactly rows * width * 3 bytes: a read behind an odd frame's last row is the sanitizer's.
 * Every record length the format has must have occurred, in the family that is there to make it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_delta_half.h"
#include "trt_host.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_random(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 40);
}

static int g_failures;
static long g_cases;
#define FAIL(...)                                                   \
    do                                                              \
    {                                                               \
        if (g_failures++ < 20)                                      \
        {                                                           \
            fprintf(stderr, "ansi_delta_half_check: " __VA_ARGS__); \
            fputc('\n', stderr);                                    \
        }                                                           \
    } while (0)

enum
{
    NOTHING,       /* nothing changed */
    ALL_DIFFERENT, /* every pixel changed, all horizontal neighbours different: the bound (an even frame's) */
    ALL_ONE,       /* every pixel changed, one colour: both colours equal the left neighbour's, the 3- and 7-byte records */
    ALTERNATE,     /* every other pixel */
    FIRST_ONLY,
    LAST_ONLY,
    ACROSS_ROWS,   /* a run into a pixel row's last cell, one from the next row's first cell, the same colour */
    LEFT_COLOUR,   /* a changed pixel whose new colour is its unchanged left neighbour's */
    RANDOM_TWO_001, RANDOM_TWO_40, RANDOM_TWO_99, RANDOM_FULL_001, RANDOM_FULL_40, RANDOM_FULL_99,
    UPPER_ONLY,    /* only the cells' upper pixel rows changed */
    LOWER_ONLY,    /* only the lower ones */
    SAME_UPPER,    /* every cell changed, the upper colour equals the left neighbour's while the lower differs: 22 and 26 bytes */
    SAME_LOWER,    /* the converse */
    FAMILIES
};
static const char *const k_family[FAMILIES] = {"nothing", "all different", "all one colour", "alternate", "first only", "last only", "across rows", "left colour",
                                               "random two 0.01", "random two 0.4", "random two 0.99", "random full 0.01", "random full 0.4", "random full 0.99",
                                               "upper only", "lower only", "same upper", "same lower"};
static const unsigned k_lengths[8] = {3, 7, 22, 26, 39, 43, 53, 57};
static unsigned g_seen[FAMILIES]; /* bit i: a record of k_lengths[i] bytes occurred */

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

/* pixel row r: every pixel another colour than it was and than its new left neighbour */
static void row_all_different(const unsigned char *shown, unsigned char *next, int width, int r)
{
    for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
        put(next, p, other_than(get(shown, p), p % width ? get(next, p - 1) : get(shown, p)));
}
/* pixel row r: every pixel changed, to one colour */
static void row_all_one(unsigned char *shown, unsigned char *next, int width, int r)
{
    for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
        put(shown, p, 0x102030u + (unsigned)(p & 1)), put(next, p, 0xa0b0c0u);
}

static void make_frames(int family, int width, int rows, unsigned char *shown, unsigned char *next)
{
    const long long cells = (long long)width * rows; /* pixels */
    for (long long p = 0; p < cells; p++)
        put(shown, p, next_random() & 0xffffffu);
    memcpy(next, shown, (size_t)cells * 3);
    switch (family)
    {
    case NOTHING:
        break;
    case ALL_DIFFERENT:
        for (int r = 0; r < rows; r++)
            row_all_different(shown, next, width, r);
        break;
    case ALL_ONE:
        for (int r = 0; r < rows; r++)
            row_all_one(shown, next, width, r);
        break;
    case UPPER_ONLY:
        for (int r = 0; r < rows; r += 2)
            row_all_different(shown, next, width, r);
        break;
    case LOWER_ONLY:
        for (int r = 1; r < rows; r += 2)
            row_all_different(shown, next, width, r);
        break;
    case SAME_UPPER:
    case SAME_LOWER:
        for (int r = 0; r < rows; r++)
            if ((r & 1) == (family == SAME_LOWER))
                row_all_one(shown, next, width, r);
            else
                row_all_different(shown, next, width, r);
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
        { /* the last two pixels of row r (where there are two) and the first two of row r + 1 */
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

/* the pixels of cell q = t * width + col of a frame: the lower one is black, and not read, behind an odd frame's last row */
static unsigned upper_of(const unsigned char *frame, int width, long long q) { return get(frame, 2 * (q / width) * width + q % width); }
static unsigned lower_of(const unsigned char *frame, int width, int rows, long long q)
{
    return 2 * (q / width) + 1 < rows ? get(frame, (2 * (q / width) + 1) * width + q % width) : 0u;
}
static int changed_at(const unsigned char *shown, const unsigned char *next, int width, int rows, long long q)
{
    return upper_of(shown, width, q) != upper_of(next, width, q) || lower_of(shown, width, rows, q) != lower_of(next, width, rows, q);
}

/* what delta_half_cells of trt_ansi_delta_half.hpp gives a lane for cell q */
static trt_delta_half_flags flags_of(const unsigned char *shown, const unsigned char *next, int width, int rows, long long q)
{
    const int col = (int)(q % width);
    trt_delta_half_flags f;
    f.changed = changed_at(shown, next, width, rows, q);
    f.changed_left = col > 0 && changed_at(shown, next, width, rows, q - 1);
    f.changed_right = col + 1 < width && changed_at(shown, next, width, rows, q + 1);
    f.same_upper = col > 0 && upper_of(next, width, q) == upper_of(next, width, q - 1);
    f.same_lower = col > 0 && lower_of(next, width, rows, q) == lower_of(next, width, rows, q - 1);
    return f;
}

static void check(int family, int width, int rows)
{
    const long long pixels = (long long)width * rows, trows = trt_ansi_half_text_rows(rows), cells = (long long)width * trows;
    const unsigned long long bound = trt_delta_half_bound(width, rows), tiles = trt_delta_tiles((unsigned long long)cells);
    unsigned char *shown = (unsigned char *)malloc((size_t)pixels * 3), *next = (unsigned char *)malloc((size_t)pixels * 3); /* to the byte */
    char *want = (char *)malloc((size_t)bound);
    unsigned char *got = (unsigned char *)calloc((size_t)bound + 64, 1), *stores = (unsigned char *)calloc((size_t)bound + 64, 1);
    unsigned *tile_bytes = (unsigned *)calloc((size_t)tiles, sizeof *tile_bytes);
    unsigned long long *tile_at = (unsigned long long *)calloc((size_t)tiles, sizeof *tile_at);
    size_t want_bytes = 0;
    g_cases++;
    make_frames(family, width, rows, shown, next);
    if (bound != (unsigned long long)trows * (39ull * width + 18) || trt_delta_half_capacity(width, rows) != bound || bound <= trt_ansi_half_text_bytes(width, rows))
        FAIL("%d x %d: bound %llu, capacity %llu", width, rows, bound, trt_delta_half_capacity(width, rows));
    if (trt_emitter_delta_half_rgb8(shown, next, width, rows, want, (size_t)bound, &want_bytes) != TRT_HOST_OK)
        FAIL("%s %d x %d: the emitter refused", k_family[family], width, rows);
    if (trt_emitter_delta_half_rgb8(shown, next, width, rows, want, (size_t)bound - 1, &want_bytes) != TRT_HOST_ERR_ARGUMENT)
        FAIL("%d x %d: the emitter took a capacity below the bound", width, rows);
    /* measure: a sum per tile */
    for (unsigned long long t = 0; t < tiles; t++)
    {
        for (long long q = (long long)t * TRT_DELTA_TILE; q < (long long)(t + 1) * TRT_DELTA_TILE && q < cells; q++)
        {
            const trt_delta_half_flags f = flags_of(shown, next, width, rows, q);
            const unsigned n = trt_delta_half_record_bytes(&f);
            int known = n == 0;
            for (int i = 0; i < 8; i++)
                if (n == k_lengths[i])
                    known = 1, g_seen[family] |= 1u << i;
            if (!known)
                FAIL("%s %d x %d: a record of %u bytes at cell %lld", k_family[family], width, rows, n, q);
            tile_bytes[t] += n;
        }
        if (tile_bytes[t] > TRT_DELTA_TILE * TRT_DELTA_HALF_RECORD_MAX)
            FAIL("%s %d x %d: tile %llu has %u bytes", k_family[family], width, rows, t, tile_bytes[t]);
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
                const long long q = (long long)t * TRT_DELTA_TILE + (long long)lane * TRT_DELTA_LANE_CELLS + j;
                if (q >= cells)
                    continue;
                const trt_delta_half_flags f = flags_of(shown, next, width, rows, q);
                const unsigned n = trt_delta_half_record_bytes(&f);
                for (unsigned k = 0; k < n; k++)
                {
                    if (at + k >= bound)
                    {
                        FAIL("%s %d x %d: a store behind the bound", k_family[family], width, rows);
                        break;
                    }
                    got[at + k] = (unsigned char)trt_delta_half_record_byte(k, (int)(q / width), (int)(q % width), upper_of(next, width, q), lower_of(next, width, rows, q), &f);
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
    /* an odd frame's last text row has one lower colour, black: behind its first cell a record sets the upper colour alone, 17 bytes fewer */
    if (family == ALL_DIFFERENT && length != bound - (rows & 1 ? 17ull * (width - 1) : 0ull))
        FAIL("all different %d x %d: %llu bytes, the bound is %llu", width, rows, length, bound);
    if (family == NOTHING && length != 0)
        FAIL("nothing changed %d x %d: %llu bytes", width, rows, length);
    if (family == ALL_ONE && length != (unsigned long long)trows * (3ull * width + 14 + 36 + 4))
        FAIL("all one colour %d x %d: %llu bytes", width, rows, length);
    if ((family == SAME_UPPER || family == SAME_LOWER) && rows % 2 == 0 && length != (unsigned long long)trows * (14 + 36 + 19ull * (width - 1) + 3ull * width + 4))
        FAIL("%s %d x %d: %llu bytes", k_family[family], width, rows, length);
    if (family == UPPER_ONLY && length < (unsigned long long)trows * (14 + 36 + 19ull * (width - 1) + 3ull * width + 4))
        FAIL("upper only %d x %d: %llu bytes: every cell has a record that sets the upper colour", width, rows, length);
    if (family == LOWER_ONLY && length < (unsigned long long)(rows / 2) * (14 + 36 + 19ull * (width - 1) + 3ull * width + 4))
        FAIL("lower only %d x %d: %llu bytes: every cell with a lower pixel has a record that sets the lower colour", width, rows, length);
    if (family == LOWER_ONLY && rows == 1 && length != 0)
        FAIL("lower only %d x 1: %llu bytes of a frame without a lower row", width, length);
    free(shown), free(next), free(want), free(got), free(stores), free(tile_bytes), free(tile_at);
}

/* bits of k_lengths that the family is there to make */
static void must_have_seen(int family, unsigned bits)
{
    if ((g_seen[family] & bits) != bits)
        FAIL("%s: record lengths seen %#x, wanted %#x", k_family[family], g_seen[family], bits);
}

int main(void)
{
    /* the limits, the bound, the size pins */
    unsigned char px[6] = {0, 0, 0, 1, 2, 3};
    char text[128];
    size_t n = 0;
    if (!trt_delta_half_size_ok(99999, 199998) || !trt_delta_half_size_ok(1, 199997) || trt_delta_half_size_ok(100000, 1) || trt_delta_half_size_ok(1, 199999) ||
        trt_delta_half_size_ok(0, 1) || trt_delta_half_size_ok(1, 0))
        FAIL("the limits");
    if (trt_delta_half_capacity(1, 1) != 57 || trt_delta_half_capacity(160, 48) != 150192 || trt_delta_half_capacity(160, 47) != 150192 || trt_delta_half_capacity(100000, 1) != 0 ||
        trt_delta_half_capacity(1, 199999) != 0 || trt_delta_half_capacity(0, 1) != 0 || trt_delta_half_bound(99999, 199998) != 99999ull * (39ull * 99999 + 18))
        FAIL("the size pins");
    if (TRT_DELTA_HALF_RECORD_MAX != 57 || TRT_DELTA_TILE * TRT_DELTA_HALF_RECORD_MAX != 58368)
        FAIL("the constants");
    if (trt_emitter_delta_half_rgb8(px, px + 3, 100000, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta_half_rgb8(px, px + 3, 1, 199999, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta_half_rgb8(px, px + 3, 0, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta_half_rgb8(NULL, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta_half_rgb8(px, NULL, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta_half_rgb8(px, px + 3, 1, 1, NULL, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta_half_rgb8(px, px + 3, 1, 1, text, sizeof text, NULL) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta_half_rgb8(px, px + 3, 1, 1, text, 56, &n) != TRT_HOST_ERR_ARGUMENT)
        FAIL("the emitter's refusals");
    /* the one cell, spelled out: the pixel is the UPPER half, the foreground */
    if (trt_emitter_delta_half_rgb8(px, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_OK || n != 57 ||
        memcmp(text, "\033[00001;00001H\033[38;2;001;002;003;48;2;000;000;000m\xe2\x96\x80\033[0m", 57) != 0)
        FAIL("the record of a 1 x 1 screen");
    /* the last cell of the largest screen, and the two single colours */
    {
        const trt_delta_half_flags lone = {0, 1, 0, 0, 0}, upper = {1, 1, 1, 0, 1}, lower = {1, 1, 0, 1, 0};
        char record[64] = {0};
        for (unsigned k = 0; k < trt_delta_half_record_bytes(&lone); k++)
            record[k] = (char)trt_delta_half_record_byte(k, 99998, 99998, 0x0c22ffu, 0x010203u, &lone);
        if (strcmp(record, "\033[99999;99999H\033[38;2;255;034;012;48;2;003;002;001m\xe2\x96\x80\033[0m") != 0)
            FAIL("the record of the last cell of the largest screen");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta_half_record_bytes(&upper); k++)
            record[k] = (char)trt_delta_half_record_byte(k, 0, 1, 0x0c22ffu, 0x010203u, &upper);
        if (strcmp(record, "\033[38;2;255;034;012m\xe2\x96\x80") != 0)
            FAIL("the record that sets the upper colour alone");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta_half_record_bytes(&lower); k++)
            record[k] = (char)trt_delta_half_record_byte(k, 0, 1, 0x0c22ffu, 0x010203u, &lower);
        if (strcmp(record, "\033[48;2;003;002;001m\xe2\x96\x80\033[0m") != 0)
            FAIL("the record that sets the lower colour alone");
    }
    for (int family = 0; family < FAMILIES; family++)
    {
        for (int width = 1; width <= 70; width++)
            for (int rows = 1; rows <= 5; rows++)
                check(family, width, rows);
        check(family, 160, 47);
        check(family, 160, 48);
        check(family, 480, 280);
    }
    /* k_lengths: 3, 7, 22, 26, 39, 43, 53, 57 are bits 0..7 */
    must_have_seen(ALL_ONE, 0x01 | 0x02 | 0x40 | 0x80);       /* both colours the left neighbour's: 3 and 7 behind a run's first cell */
    must_have_seen(SAME_UPPER, 0x04 | 0x08 | 0x40 | 0x80);    /* one colour: 22 and 26 */
    must_have_seen(SAME_LOWER, 0x04 | 0x08 | 0x40 | 0x80);
    must_have_seen(UPPER_ONLY, 0x04 | 0x08 | 0x10 | 0x20);    /* 22 and 26 in an odd frame's last text row, whose lower colour is black throughout */
    must_have_seen(LOWER_ONLY, 0x10 | 0x20 | 0x40 | 0x80);    /* the unchanged upper colours are random: both differ from the left neighbour's */
    must_have_seen(ALL_DIFFERENT, 0x10 | 0x20 | 0x40 | 0x80); /* both: 39 and 43; a run's first cell: 53 and, alone in its row, 57 */
    if (g_failures)
    {
        fprintf(stderr, "ansi_delta_half_check: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("ansi_delta_half_check: ok (%ld cases)\n", g_cases);
    return 0;
}
