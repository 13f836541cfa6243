/* ansi_delta_half_check.c -- csrc/trt_ansi_delta_half.h, the format of the delta text between two RGB8 frames in half-block cells and the
 * walk the device kernels (csrc/trt_ansi_delta.hpp) load their cells and place their records by, compiled for the host and held against the
 * sequential emitter trt_emitter_delta_half_rgb8 (csrc/host/trt_emit.c), which does not use the header.  A program of its own:
 * tests/test_ansi_delta_half_layout.py builds and runs it plain and under -fsanitize=address,undefined.
 *
 * For every width 1..70 x rows 1..5 (odd and even frames, one text row), 160 x 47, 160 x 48 and 480 x 280, and every pattern family,
 * check() of ansi_delta_check.h assembles the text by calling the kernels' own walk, trt_delta_half_lane_cells and trt_delta_half_lane_byte,
 * for every tile and every thread -- the lanes' totals summed per tile, the exclusive scan of the tiles' sums in turns of
 * TRT_DELTA_SCAN_BLOCK, each lane behind the lanes before it -- into a buffer with a count per byte: the text equals the emitter's to the
 * byte and in length, every byte below the length was stored exactly once and none at or behind it, the length is within
 * trt_delta_half_bound (and equals it where every cell changed and both colours differ from the left neighbour's everywhere), and the
 * limits hold.  The frames are allocated at exactly rows * width * 3 bytes: a load behind an odd frame's last row is the sanitizer's.
 * Every record length the format has must have occurred, in the family that is there to make it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_delta_half.h"
#include "trt_host.h"

#define CHECK_NAME "ansi_delta_half_check"
#define KIND_LANE trt_delta_half_lane
#define KIND_LANE_CELLS trt_delta_half_lane_cells
#define KIND_LANE_BYTE trt_delta_half_lane_byte
#define KIND_EMITTER trt_emitter_delta_half_rgb8
#define KIND_BOUND trt_delta_half_bound
#define KIND_TEXT_ROWS(rows) trt_ansi_half_text_rows(rows)
#define KIND_RECORD_MAX TRT_DELTA_HALF_RECORD_MAX
#define LENGTHS 8
static const unsigned k_lengths[LENGTHS] = {3, 7, 22, 26, 39, 43, 53, 57};

#include "ansi_delta_check.h"

static void kind_verdicts(int family, int width, int rows, unsigned long long length, unsigned long long bound, const unsigned char *shown, const unsigned char *next)
{
    const long long trows = trt_ansi_half_text_rows(rows);
    (void)shown, (void)next;
    if (bound != (unsigned long long)trows * (39ull * width + 18) || trt_delta_half_capacity(width, rows) != bound || bound <= trt_ansi_half_text_bytes(width, rows))
        FAIL("%d x %d: bound %llu, capacity %llu", width, rows, bound, trt_delta_half_capacity(width, rows));
    /* an odd frame's last text row has one lower colour, black: behind its first cell a record sets the upper colour alone, 17 bytes fewer */
    if (family == ALL_DIFFERENT && length != bound - (rows & 1 ? 17ull * (width - 1) : 0ull))
        FAIL("all different %d x %d: %llu bytes, the bound is %llu", width, rows, length, bound);
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
    for (int family = 0; family < ALL_FAMILIES; family++)
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
    return verdict();
}
