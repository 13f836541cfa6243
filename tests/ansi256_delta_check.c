/* ansi256_delta_check.c -- csrc/trt_ansi256_delta.h, the format of the delta text between two RGB8 frames in the xterm 256-colour palette
 * (the full text's cells) and the walk the device kernels (csrc/trt_ansi_delta.hpp) load their cells and place their records by, compiled
 * for the host and held against the sequential emitter trt_emitter_delta256_rgb8 (csrc/host/trt_emit.c), which uses neither the header nor
 * the closed form of the palette map.  A program of its own: tests/test_ansi256_delta_layout.py builds and runs it plain and under
 * -fsanitize=address,undefined.
 *
 * For widths 1..5, 63..65 and 1023..1025 x rows 1, 2, 3 and 7, and 131 x 17 (seventeen rows over three tiles, rows that straddle a
 * tile's edge), every family of ansi256_delta_check.h in both modes: the text equals the emitter's to the byte and in length, every byte
 * below the length was stored exactly once and none at or behind it, nothing behind a frame was loaded (the sanitizer's), the length
 * is within trt_delta256_bound and EQUALS it in the "longest" family.  The bound itself is held against an enumeration of every pattern of
 * changed cells and equal neighbours of a row of 1..12 cells.  Every record length the format has must have occurred.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi256_delta.h"
#include "trt_host.h"

#define CHECK_NAME "ansi256_delta_check"
#define KIND_LANE trt_delta256_lane
#define KIND_LANE_CELLS trt_delta256_lane_cells
#define KIND_LANE_BYTE trt_delta256_lane_byte
#define KIND_EMITTER trt_emitter_delta256_rgb8
#define KIND_BOUND trt_delta256_bound
#define KIND_TEXT_ROWS(rows) (rows)
#define KIND_RECORD_MAX TRT_DELTA256_RECORD_MAX
#define KIND_RGB_EMITTER trt_emitter_delta_rgb8
#define KIND_RGB_MOST(width, rows) trt_delta_bound(width, rows) /* the 24-bit text of a pair whose every cell changed, all neighbours different */
#define KIND_RGB_BOUND trt_delta_bound
#define KIND_ROW_BOUND trt_delta256_row_bound
#define KIND_STATES 3 /* unchanged; changed, the left neighbour's index; changed, another index */
#define LENGTHS 6
static const unsigned k_lengths[LENGTHS] = {2, 6, 13, 17, 27, 31};

#include "ansi256_delta_check.h"

static unsigned kind_cell_bytes(int changed_left, int state, int changed_right)
{
    const trt_delta_flags f = {changed_left, state != 0, changed_right, state == 1};
    return trt_delta256_record_bytes(&f);
}

/* changed and unchanged cells in turn, from column 0; an even row's last two cells both, to different indices */
static void kind_longest(unsigned char *shown, unsigned char *next, int width, int rows)
{
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < width; c++)
            if (c % 2 == 0 || c == width - 1)
            {
                const long long p = (long long)r * width + c;
                unsigned to;
                do
                    to = entry_colour(16 + next_random() % 240);
                while (index_of(to) == index_of(get(shown, p)) || (c > 0 && index_of(to) == index_of(get(next, p - 1))));
                put(next, p, to);
            }
}

static void kind_verdicts(int family, int width, int rows, unsigned long long length, unsigned long long bound, const unsigned char *shown, const unsigned char *next)
{
    (void)shown, (void)next;
    if (bound != (unsigned long long)rows * (13ull * width + 13 + 5ull * ((width + 1) / 2)) || trt_delta256_capacity(width, rows) != bound ||
        bound <= trt_ansi256_text_bytes(width, rows))
        FAIL("%d x %d: bound %llu, capacity %llu", width, rows, bound, trt_delta256_capacity(width, rows));
    if (family == LONGEST && length != bound)
        FAIL("longest %d x %d: %llu bytes, the bound is %llu", width, rows, length, bound);
    if (family == INDEX_RUN && length != (unsigned long long)rows * (14 + 11 + 2ull * width + 4))
        FAIL("index run %d x %d: %llu bytes: one colour a row", width, rows, length);
    if (family == ALL_ONE && length != (unsigned long long)rows * (14 + 11 + 2ull * width + 4))
        FAIL("all one colour %d x %d: %llu bytes", width, rows, length);
    if (family == ALL_DIFFERENT && g_entries && length != (unsigned long long)rows * (18 + 13ull * width))
        FAIL("all different %d x %d: %llu bytes: one run a row, a colour a cell", width, rows, length);
}

int main(void)
{
    static const int widths[] = {1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025}, heights[] = {1, 2, 3, 7};
    unsigned char px[6] = {0, 0, 0, 1, 2, 200};
    char text[128];
    size_t n = 0;
    if (!trt_delta256_size_ok(49999, 99999) || trt_delta256_size_ok(50000, 1) || trt_delta256_size_ok(1, 100000) || trt_delta256_size_ok(0, 1) || trt_delta256_size_ok(1, 0))
        FAIL("the limits");
    if (trt_delta256_bound(1, 1) != 31 || trt_delta256_bound(2, 1) != 44 || trt_delta256_capacity(1, 1) != 31 || trt_delta256_capacity(50000, 1) != 0 ||
        trt_delta256_capacity(1, 100000) != 0 || trt_delta256_capacity(0, 1) != 0 || trt_delta256_capacity(1, -1) != 0 ||
        trt_delta256_bound(49999, 99999) != 99999ull * (13ull * 49999 + 13 + 5ull * 25000))
        FAIL("the size pins");
    if (TRT_DELTA256_RECORD_MAX != 31)
        FAIL("the constants");
    if (trt_emitter_delta256_rgb8(px, px + 3, 50000, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_rgb8(px, px + 3, 1, 100000, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_rgb8(px, px + 3, 0, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta256_rgb8(NULL, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_rgb8(px, NULL, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta256_rgb8(px, px + 3, 1, 1, NULL, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_rgb8(px, px + 3, 1, 1, text, sizeof text, NULL) != TRT_HOST_ERR_ARGUMENT || trt_emitter_delta256_rgb8(px, px + 3, 1, 1, text, 30, &n) != TRT_HOST_ERR_ARGUMENT)
        FAIL("the emitter's refusals");
    /* the one cell, spelled out: (1, 2, 200) is nearest to the cube's (0, 0, 215), entry 16 + 4 = 20 */
    if (trt_emitter_delta256_rgb8(px, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_OK || n != 31 || memcmp(text, "\033[00001;00001H\033[48;5;020m  \033[0m", 31) != 0)
        FAIL("the record of a 1 x 1 screen");
    {
        const trt_delta_flags lone = {0, 1, 0, 0}, inside = {1, 1, 1, 1}, last = {1, 1, 0, 0};
        char record[64] = {0};
        for (unsigned k = 0; k < trt_delta256_record_bytes(&lone); k++)
            record[k] = (char)trt_delta256_record_byte(k, 99998, 49998, 255, &lone);
        if (strcmp(record, "\033[99999;99997H\033[48;5;255m  \033[0m") != 0)
            FAIL("the record of the last cell of the largest screen");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta256_record_bytes(&inside); k++)
            record[k] = (char)trt_delta256_record_byte(k, 0, 1, 16, &inside);
        if (strcmp(record, "  ") != 0)
            FAIL("the record inside a run of one index");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta256_record_bytes(&last); k++)
            record[k] = (char)trt_delta256_record_byte(k, 0, 1, 16, &last);
        if (strcmp(record, "\033[48;5;016m  \033[0m") != 0)
            FAIL("the record that ends a run with another index");
    }
    check_bound_by_enumeration();
    for (g_entries = 0; g_entries < 2; g_entries++)
        for (int family = 0; family < ALL_FAMILIES; family++)
        {
            for (unsigned w = 0; w < sizeof widths / sizeof widths[0]; w++)
                for (unsigned h = 0; h < sizeof heights / sizeof heights[0]; h++)
                    check(family, widths[w], heights[h]);
            check(family, 131, 17);
        }
    /* k_lengths: 2, 6, 13, 17, 27, 31 are bits 0..5 */
    must_have_seen(INDEX_RUN, 0x01 | 0x02 | 0x10 | 0x20); /* the colour at the run's start alone: 2 and 6 behind it */
    must_have_seen(ALL_DIFFERENT, 0x04 | 0x08 | 0x10 | 0x20);
    must_have_seen(LONGEST, 0x20 | 0x10 | 0x08); /* runs of one; an even row's run of two: 27 and 17 */
    return verdict();
}
