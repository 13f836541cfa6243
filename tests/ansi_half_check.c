/* ansi_half_check.c -- csrc/trt_ansi_half.h, the format of a frame's half-block terminal text, with the position map and the lane map of the device
 * pass that writes it (csrc/trt_text_map.h), compiled for the host and held against the sequential emitter trt_emitter_half_rgb8
 * (csrc/host/trt_emit.c).  A program of its own: tests/test_ansi_half_layout.py builds and runs it plain and under -fsanitize=address,undefined.
 * tests/ansi_text_check.h says what is checked, here for every width 1..70 x rows 1..5 and for 160 x 48, 480 x 280 and 1920 x 1080:
 *
 *  (1) layout: 6 prefix bytes, every byte of every cell, 5 end bytes per text row, no NUL;
 *  (2) lane map: two registers a lane, both read from ONE lane a word; every lane's cell (trt_ansi_half_lane_cell) is the wave's first plus
 *      the lane.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_half.h"
#include "trt_host.h"

#define CHECK_NAME "ansi_half_check"
#define KIND trt_ansi_half_kind()
#define KIND_SPAN_CELLS TRT_ANSI_HALF_SPAN_CELLS
#define KIND_WAVE_WORDS TRT_ANSI_HALF_WAVE_WORDS
#define KIND_TEXT_ROWS(rows) trt_ansi_half_text_rows(rows)
#define KIND_TEXT_BYTES(width, rows) trt_ansi_half_text_bytes(width, rows)
#define KIND_LONE_VALUE(position, bytes) trt_ansi_half_lone_value(position, bytes)
#define KIND_MIN_BYTES 50
#define KIND_ROWS 5
#define KIND_MAP_ALL 1
static const int k_larger[][2] = {{160, 48}, {480, 280}, {1920, 1080}};
static const int k_mapped[][2] = {{1, 1}}; /* every size is mapped already */

typedef struct
{
    unsigned upper, lower;
} kind_held, kind_seen; /* a cell's two pixels */

#include "ansi_text_check.h"

/* the two pixels of the cell (trow, col): what a lane of the device pass forms; the lower one of an odd frame's last row is 0 and is not read */
static kind_held cell_pixels(const unsigned char *rgb, int width, int rows, long long trow, int col)
{
    kind_held cell = {0u, 0u};
    if (2 * trow < rows)
    {
        const long long p = 2 * trow * width + col;
        cell.upper = packed(rgb, p);
        if (2 * trow + 1 < rows)
            cell.lower = packed(rgb, p + width);
    }
    return cell;
}

static char *emitter_text(int width, int rows, const unsigned char *rgb, size_t *size)
{
    const size_t room = (size_t)trt_ansi_half_text_bytes(width, rows);
    char *text = (char *)malloc(room);
    if (!text || trt_emitter_half_rgb8(rgb, width, rows, text, room, size) != TRT_HOST_OK)
    {
        fprintf(stderr, "ansi_half_check: no emitter text for %d x %d\n", width, rows);
        exit(2);
    }
    return text;
}

static unsigned kind_position_byte(const trt_text_at *at, int width, int rows, const unsigned char *rgb)
{
    kind_held cell = {0xABCDEFu, 0x123456u};
    if (at->r >= 0 && at->row < trt_ansi_half_text_rows(rows))
        cell = cell_pixels(rgb, width, rows, at->row, at->col);
    return trt_ansi_half_byte(at, cell.upper, cell.lower);
}

static kind_held kind_hold(const trt_text_at *from, int lane, int width, int rows, unsigned width_magic, const unsigned char *rgb)
{
    long long trow;
    int col;
    if (width_magic != trt_ansi_half_width_magic(width))
        FAIL("width %d: the width's magic", width);
    trt_ansi_half_lane_cell(from, lane, width, width_magic, &trow, &col);
    if (trow * width + col != trt_text_cell(from, width) + lane || col < 0 || col >= width)
        FAIL("%d x %d: lane %d holds row %lld col %d, its cell is %lld", width, rows, lane, trow, col, trt_text_cell(from, width) + lane);
    return cell_pixels(rgb, width, rows, trow, col);
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
    return trt_ansi_half_byte(at, shown.upper, shown.lower);
}

static void kind_constants(void)
{
    if (trt_ansi_half_text_bytes(0, 5) || trt_ansi_half_text_bytes(5, 0) || trt_ansi_half_text_bytes(-1, -1) || trt_ansi_half_text_bytes(160, 48) != 149886 ||
        trt_ansi_half_text_bytes(480, 280) != 2621506 || trt_ansi_half_text_bytes(1, 1) != 50)
        FAIL("trt_ansi_half_text_bytes of an empty screen, of 1 x 1, of 160 x 48 or of 480 x 280");
}
