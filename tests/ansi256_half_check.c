/* ansi256_half_check.c -- csrc/trt_ansi256_half.h, the format of a frame's half-block terminal text in the xterm 256-colour palette, with the
 * palette's closed form (csrc/trt_xterm256.h) and the position map and the lane map of the device pass that writes it (csrc/trt_text_map.h),
 * compiled for the host and held against the sequential emitter trt_emitter_ansi256_half_rgb8 (csrc/host/trt_emit.c), which finds its indices by
 * the 240-entry search.  A program of its own: tests/test_ansi256_layout.py builds and runs it plain and under -fsanitize=address,undefined.
 * tests/ansi_text_check.h says what is checked, here for every width 1..70 x rows 1..3 and for the widths 40, 55..61, 63, 64, 65, 67 and 130 --
 * either side of the switch from rows shorter than a span (1280 bytes: 56 cells) to longer ones and of trt_ansi256_half_lane_cell's at width 64
 * -- x rows 1, 2, 3 and 13, and for 160 x 48 and 480 x 280:
 *
 *  (1) layout: 6 prefix bytes, every byte of every cell, 5 end bytes per text row, no NUL; 016 behind the last row of an odd frame;
 *  (2) lane map: one register a lane, two palette indices, read from ONE lane a word; five words a lane; every lane's cell
 *      (trt_ansi256_half_lane_cell) is the wave's first plus the lane.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi256_half.h" /* in front of trt_host.h: trt_xterm256_index is the header's inline function here */

#include "trt_host.h"

#define CHECK_NAME "ansi256_half_check"
#define KIND trt_ansi256_half_kind()
#define KIND_SPAN_CELLS TRT_ANSI256_HALF_SPAN_CELLS
#define KIND_WAVE_WORDS TRT_ANSI256_HALF_WAVE_WORDS
#define KIND_TEXT_ROWS(rows) trt_ansi256_half_text_rows(rows)
#define KIND_TEXT_BYTES(width, rows) trt_ansi256_half_text_bytes(width, rows)
#define KIND_LONE_VALUE(position, bytes) trt_ansi256_half_lone_value(position, bytes)
#define KIND_MIN_BYTES 34
#define KIND_ROWS 3
#define KIND_MAP_ALL 1
static const int k_larger[][2] = {{40, 13},  {55, 13}, {56, 13}, {57, 13}, {58, 13}, {59, 13}, {60, 13},  {61, 13},  {63, 13},  {64, 13},
                                  {65, 13},  {67, 13}, {1, 13},  {2, 13},  {3, 13},  {5, 13},  {130, 1},  {130, 2},  {130, 3},  {130, 13},
                                  {160, 48}, {480, 280}};
static const int k_mapped[][2] = {{1, 1}}; /* every size is mapped already */

typedef unsigned kind_held, kind_seen; /* a cell's two palette indices, upper | lower << 8 */

#include "ansi_text_check.h"

/* the two indices of the cell (trow, col): what a lane of the device pass forms; black below the last row of an odd frame and where the frame has no cell */
static kind_held cell_indices(const unsigned char *rgb, int width, int rows, long long trow, int col)
{
    unsigned upper = TRT_XTERM256_BLACK, lower = TRT_XTERM256_BLACK;
    if (2 * trow < rows)
    {
        const long long p = 2 * trow * width + col;
        upper = trt_xterm256_index_of(packed(rgb, p));
        if (2 * trow + 1 < rows)
            lower = trt_xterm256_index_of(packed(rgb, p + width));
    }
    return trt_ansi256_half_pair(upper, lower);
}

static char *emitter_text(int width, int rows, const unsigned char *rgb, size_t *size)
{
    const size_t room = (size_t)trt_ansi256_half_text_bytes(width, rows);
    char *text = (char *)malloc(room);
    if (!text || trt_emitter_ansi256_half_rgb8(rgb, width, rows, text, room, size) != TRT_HOST_OK)
    {
        fprintf(stderr, "ansi256_half_check: no emitter text for %d x %d\n", width, rows);
        exit(2);
    }
    return text;
}

static unsigned kind_position_byte(const trt_text_at *at, int width, int rows, const unsigned char *rgb)
{
    kind_held cell = 0xABCDu;
    if (at->r >= 0 && at->row < trt_ansi256_half_text_rows(rows))
        cell = cell_indices(rgb, width, rows, at->row, at->col);
    return trt_ansi256_half_byte(at, cell);
}

static kind_held kind_hold(const trt_text_at *from, int lane, int width, int rows, unsigned width_magic, const unsigned char *rgb)
{
    long long trow;
    int col;
    if (width_magic != trt_ansi256_half_width_magic(width))
        FAIL("width %d: the width's magic", width);
    trt_ansi256_half_lane_cell(from, lane, width, width_magic, &trow, &col);
    if (trow * width + col != trt_text_cell(from, width) + lane || col < 0 || col >= width)
        FAIL("%d x %d: lane %d holds row %lld col %d, its cell is %lld", width, rows, lane, trow, col, trt_text_cell(from, width) + lane);
    return cell_indices(rgb, width, rows, trow, col);
}

static kind_seen kind_colours(const trt_text_at *at, const trt_text_at *last, const trt_text_at *from, const kind_held *mine, int width, long long *rel_first,
                              long long *rel_last)
{
    (void)last; /* every digit of a word belongs to its first byte's cell */
    *rel_first = *rel_last = trt_text_cell(at, width) - trt_text_cell(from, width);
    return mine[(int)*rel_first & 63];
}

static unsigned kind_byte(const trt_text_at *at, int rows, kind_seen shown, unsigned other)
{
    (void)rows, (void)other;
    return trt_ansi256_half_byte(at, shown);
}

static void kind_constants(void)
{
    if (trt_ansi256_half_text_bytes(0, 5) || trt_ansi256_half_text_bytes(5, 0) || trt_ansi256_half_text_bytes(-1, -1) || trt_ansi256_half_text_bytes(-4, 3) ||
        trt_ansi256_half_text_bytes(4, -3) || trt_ansi256_half_text_bytes(160, 48) != 6 + (23 * 160 + 5) * 24 ||
        trt_ansi256_half_text_bytes(1920, 1081) != 6ull + (23ull * 1920 + 5) * 541 || trt_ansi256_half_text_bytes(1, 1) != 34)
        FAIL("trt_ansi256_half_text_bytes of an empty screen, of 1 x 1, of 160 x 48 or of 1920 x 1081");
    if (TRT_ANSI256_HALF_SPAN_CELLS != 57 || TRT_TEXT_SPAN_CELLS(TRT_ANSI256_HALF_CELL, TRT_ANSI256_HALF_WAVE_WORDS + 64) <= 64)
        FAIL("five words a lane are the most whose cells fit a wave's lanes");
}
