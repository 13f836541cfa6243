/* ansi256_delta_half_check.c -- csrc/trt_ansi256_delta_half.h, the format of the delta text between two RGB8 frames in half-block cells in
 * the xterm 256-colour palette and the walk the device kernels (csrc/trt_ansi_delta.hpp) load their cells and place their records by,
 * compiled for the host and held against the sequential emitter trt_emitter_delta256_half_rgb8 (csrc/host/trt_emit.c), which uses
 * neither the header nor the closed form of the palette map.  A program of its own: tests/test_ansi256_delta_layout.py builds and runs it
 * plain and under -fsanitize=address,undefined.
 *
 * The sizes, families and checks of ansi256_delta_check.c; rows 1, 3, 7 and 17 are odd frames, whose last text row has no lower pixels:
 * the frames are allocated to the byte, so a load of that row is the sanitizer's.  The "longest" family -- every cell changed, both
 * indices other than the left neighbour's -- reaches trt_delta256_half_bound in an even frame; an odd frame's last text row has one
 * lower index, black, and is 9 bytes a cell behind the first shorter.  The bound is held against an enumeration of every pattern of
 * changed cells and equal neighbours of a text row of 1..12 cells.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi256_delta_half.h"
#include "trt_host.h"

#define CHECK_NAME "ansi256_delta_half_check"
#define KIND_LANE trt_delta256_half_lane
#define KIND_LANE_CELLS trt_delta256_half_lane_cells
#define KIND_LANE_BYTE trt_delta256_half_lane_byte
#define KIND_EMITTER trt_emitter_delta256_half_rgb8
#define KIND_BOUND trt_delta256_half_bound
#define KIND_TEXT_ROWS(rows) trt_ansi256_half_text_rows(rows)
#define KIND_RECORD_MAX TRT_DELTA256_HALF_RECORD_MAX
#define KIND_RGB_EMITTER trt_emitter_delta_half_rgb8
/* the 24-bit text of a pair whose every pixel changed, all neighbours different: its bound, but for an odd frame's last text row */
#define KIND_RGB_MOST(width, rows) (trt_delta_half_bound(width, rows) - ((rows) & 1 ? 17ull * ((width) - 1) : 0ull))
#define KIND_RGB_BOUND trt_delta_half_bound
#define KIND_ROW_BOUND trt_delta256_half_row_bound
#define KIND_STATES 5 /* unchanged; changed with both indices, the upper, the lower, neither the left neighbour's */
#define LENGTHS 8
static const unsigned k_lengths[LENGTHS] = {3, 7, 14, 18, 23, 27, 37, 41};

#include "ansi256_delta_check.h"

static unsigned kind_cell_bytes(int changed_left, int state, int changed_right)
{
    const trt_delta_half_flags f = {changed_left, state != 0, changed_right, state == 1 || state == 2, state == 1 || state == 3};
    return trt_delta256_half_record_bytes(&f);
}

/* every pixel to an entry of another index than it had and than its new left neighbour has */
static void kind_longest(unsigned char *shown, unsigned char *next, int width, int rows)
{
    for (long long p = 0; p < (long long)width * rows; p++)
    {
        unsigned to;
        do
            to = entry_colour(16 + next_random() % 240);
        while (index_of(to) == index_of(get(shown, p)) || (p % width && index_of(to) == index_of(get(next, p - 1))));
        put(next, p, to);
    }
}

static void kind_verdicts(int family, int width, int rows, unsigned long long length, unsigned long long bound, const unsigned char *shown, const unsigned char *next)
{
    const long long trows = trt_ansi256_half_text_rows(rows);
    const unsigned long long one_colour_row = 14 + 20 + 11ull * (width - 1) + 3ull * width + 4;
    (void)shown, (void)next;
    if (bound != (unsigned long long)trows * (23ull * width + 18) || trt_delta256_half_capacity(width, rows) != bound || bound <= trt_ansi256_half_text_bytes(width, rows))
        FAIL("%d x %d: bound %llu, capacity %llu", width, rows, bound, trt_delta256_half_capacity(width, rows));
    /* an odd frame's last text row has one lower index, black: behind its first cell a record sets the upper colour alone, 9 bytes fewer */
    if ((family == LONGEST || (family == ALL_DIFFERENT && g_entries)) && length != bound - (rows & 1 ? 9ull * (width - 1) : 0ull))
        FAIL("%s %d x %d: %llu bytes, the bound is %llu", k_family[family], width, rows, length, bound);
    if ((family == INDEX_RUN || family == ALL_ONE) && length != (unsigned long long)trows * (14 + 20 + 3ull * width + 4))
        FAIL("%s %d x %d: %llu bytes: the colours at the run's start alone", k_family[family], width, rows, length);
    if ((family == SAME_UPPER || family == SAME_LOWER) && g_entries && rows % 2 == 0 && length != (unsigned long long)trows * one_colour_row)
        FAIL("%s %d x %d: %llu bytes", k_family[family], width, rows, length);
    if (family == LOWER_ONLY && rows == 1 && length != 0)
        FAIL("lower only %d x 1: %llu bytes of a frame without a lower row", width, length);
}

int main(void)
{
    static const int widths[] = {1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025}, heights[] = {1, 2, 3, 7};
    unsigned char px[6] = {0, 0, 0, 1, 2, 200};
    char text[128];
    size_t n = 0;
    if (!trt_delta256_half_size_ok(99999, 199998) || !trt_delta256_half_size_ok(1, 199997) || trt_delta256_half_size_ok(100000, 1) || trt_delta256_half_size_ok(1, 199999) ||
        trt_delta256_half_size_ok(0, 1) || trt_delta256_half_size_ok(1, 0))
        FAIL("the limits");
    if (trt_delta256_half_capacity(1, 1) != 41 || trt_delta256_half_capacity(160, 48) != 24ull * (23 * 160 + 18) || trt_delta256_half_capacity(160, 47) != 24ull * (23 * 160 + 18) ||
        trt_delta256_half_capacity(100000, 1) != 0 || trt_delta256_half_capacity(1, 199999) != 0 || trt_delta256_half_capacity(0, 1) != 0 ||
        trt_delta256_half_bound(99999, 199998) != 99999ull * (23ull * 99999 + 18))
        FAIL("the size pins");
    if (TRT_DELTA256_HALF_RECORD_MAX != 41 || TRT_DELTA_TILE * TRT_DELTA256_HALF_RECORD_MAX != 41984)
        FAIL("the constants");
    if (trt_emitter_delta256_half_rgb8(px, px + 3, 100000, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(px, px + 3, 1, 199999, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(px, px + 3, 0, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(NULL, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(px, NULL, 1, 1, text, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(px, px + 3, 1, 1, NULL, sizeof text, &n) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(px, px + 3, 1, 1, text, sizeof text, NULL) != TRT_HOST_ERR_ARGUMENT ||
        trt_emitter_delta256_half_rgb8(px, px + 3, 1, 1, text, 40, &n) != TRT_HOST_ERR_ARGUMENT)
        FAIL("the emitter's refusals");
    /* the one cell, spelled out: the pixel is the UPPER half, the foreground; behind the odd frame's row the palette's black */
    if (trt_emitter_delta256_half_rgb8(px, px + 3, 1, 1, text, sizeof text, &n) != TRT_HOST_OK || n != 41 ||
        memcmp(text, "\033[00001;00001H\033[38;5;020;48;5;016m\xe2\x96\x80\033[0m", 41) != 0)
        FAIL("the record of a 1 x 1 screen");
    {
        const trt_delta_half_flags lone = {0, 1, 0, 0, 0}, upper = {1, 1, 1, 0, 1}, lower = {1, 1, 0, 1, 0}, neither = {1, 1, 1, 1, 1};
        const unsigned pair = trt_ansi256_half_pair(255, 16);
        char record[64] = {0};
        for (unsigned k = 0; k < trt_delta256_half_record_bytes(&lone); k++)
            record[k] = (char)trt_delta256_half_record_byte(k, 99998, 99998, pair, &lone);
        if (strcmp(record, "\033[99999;99999H\033[38;5;255;48;5;016m\xe2\x96\x80\033[0m") != 0)
            FAIL("the record of the last cell of the largest screen");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta256_half_record_bytes(&upper); k++)
            record[k] = (char)trt_delta256_half_record_byte(k, 0, 1, pair, &upper);
        if (strcmp(record, "\033[38;5;255m\xe2\x96\x80") != 0)
            FAIL("the record that sets the upper colour alone");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta256_half_record_bytes(&lower); k++)
            record[k] = (char)trt_delta256_half_record_byte(k, 0, 1, pair, &lower);
        if (strcmp(record, "\033[48;5;016m\xe2\x96\x80\033[0m") != 0)
            FAIL("the record that sets the lower colour alone");
        memset(record, 0, sizeof record);
        for (unsigned k = 0; k < trt_delta256_half_record_bytes(&neither); k++)
            record[k] = (char)trt_delta256_half_record_byte(k, 0, 1, pair, &neither);
        if (strcmp(record, "\xe2\x96\x80") != 0)
            FAIL("the record that sets no colour");
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
    /* k_lengths: 3, 7, 14, 18, 23, 27, 37, 41 are bits 0..7 */
    must_have_seen(INDEX_RUN, 0x01 | 0x02 | 0x40 | 0x80);  /* both indices the left neighbour's: 3 and 7 behind a run's first cell */
    must_have_seen(SAME_UPPER, 0x04 | 0x08 | 0x40 | 0x80); /* one colour: 14 and 18 */
    must_have_seen(SAME_LOWER, 0x04 | 0x08 | 0x40 | 0x80);
    must_have_seen(LONGEST, 0x10 | 0x20 | 0x40 | 0x80); /* both: 23 and 27; a run's first cell: 37 and, alone in its row, 41 */
    return verdict();
}
