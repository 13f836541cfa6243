/* ansi_delta_check.c -- csrc/trt_ansi_delta.h, the format of the delta text between two RGB8 frames and the walk the device kernels
 * (csrc/trt_ansi_delta.hpp) load their cells and place their records by, compiled for the host and held against the sequential emitter
 * trt_emitter_delta_rgb8 (csrc/host/trt_emit.c), which does not use the header.  A program of its own: tests/test_ansi_delta_layout.py builds
 * and runs it plain and under -fsanitize=address,undefined.
 *
 * For every width 1..70 x rows 1..4, 160 x 48 and 480 x 280, and every pattern family of both kinds, check() of ansi_delta_check.h assembles
 * the text by calling the kernels' own walk, trt_delta_lane_cells and trt_delta_lane_byte, for every tile and every thread -- the lanes'
 * totals summed per tile, the exclusive scan of the tiles' sums in turns of TRT_DELTA_SCAN_BLOCK, each lane behind the lanes before it -- into
 * a buffer with a count per byte: the text equals the emitter's to the byte and in length, every byte below the length was stored exactly
 * once and none at or behind it, the length is within trt_delta_bound (and equals it where every cell changed and all neighbours differ),
 * and the limits hold.  The frames are allocated to the byte: a load behind a frame is the sanitizer's.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_delta.h"
#include "trt_host.h"

#define CHECK_NAME "ansi_delta_check"
#define KIND_LANE trt_delta_lane
#define KIND_LANE_CELLS trt_delta_lane_cells
#define KIND_LANE_BYTE trt_delta_lane_byte
#define KIND_EMITTER trt_emitter_delta_rgb8
#define KIND_BOUND trt_delta_bound
#define KIND_TEXT_ROWS(rows) (rows)
#define KIND_RECORD_MAX TRT_DELTA_RECORD_MAX
#define LENGTHS 6
static const unsigned k_lengths[LENGTHS] = {2, 6, 21, 25, 35, 39};

#include "ansi_delta_check.h"

static void kind_verdicts(int family, int width, int rows, unsigned long long length, unsigned long long bound, const unsigned char *shown, const unsigned char *next)
{
    const long long cells = (long long)width * rows;
    if (bound != (unsigned long long)rows * (21ull * width + 18))
        FAIL("%d x %d: bound %llu", width, rows, bound);
    if (family == ALL_DIFFERENT && length != bound)
        FAIL("all different %d x %d: %llu bytes, the bound is %llu", width, rows, length, bound);
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
    for (int family = 0; family < SHARED_FAMILIES; family++) /* those of both kinds */
    {
        for (int width = 1; width <= 70; width++)
            for (int rows = 1; rows <= 4; rows++)
                check(family, width, rows);
        check(family, 160, 48);
        check(family, 480, 280);
    }
    /* k_lengths: 2, 6, 21, 25, 35, 39 are bits 0..5 */
    must_have_seen(ALL_ONE, 0x01 | 0x02 | 0x10 | 0x20);       /* the colour the left neighbour's: 2 and 6 behind a run's first cell */
    must_have_seen(ALL_DIFFERENT, 0x04 | 0x08 | 0x10 | 0x20); /* a colour each: 21 and 25; a run's first cell: 35 and, alone in its row, 39 */
    return verdict();
}
