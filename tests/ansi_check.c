/* ansi_check.c -- csrc/trt_ansi.h, the format of a frame's terminal text, with the position map and the lane map of the device pass that writes it
 * (csrc/trt_text_map.h), compiled for the host and held against the host emitter (csrc/host/trt_emit.c).  A program of its own:
 * tests/test_ansi_layout.py builds and runs it plain and under -fsanitize=address,undefined.  tests/ansi_text_check.h says what is checked:
 *
 *  (1) layout, for every width 1..70 x rows 1..4 and a few larger screens: 6 prefix bytes, every byte of every cell, a newline per row, 3 NULs;
 *      the emitter's buffer after trt_emitter_patch_rgb8;
 *  (2) lane map, for the screens of k_mapped: one register a lane, two cross-lane reads a word.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi.h"
#include "trt_host.h"

#define CHECK_NAME "ansi_check"
#define KIND trt_ansi_kind()
#define KIND_SPAN_CELLS TRT_ANSI_SPAN_CELLS
#define KIND_WAVE_WORDS TRT_ANSI_WAVE_WORDS
#define KIND_TEXT_ROWS(rows) trt_ansi_text_rows(rows)
#define KIND_TEXT_BYTES(width, rows) trt_ansi_text_bytes(width, rows)
#define KIND_LONE_VALUE(position, bytes) trt_ansi_lone_value(position, bytes)
#define KIND_MIN_BYTES 35
#define KIND_ROWS 4
#define KIND_MAP_ALL 0
static const int k_larger[][2] = {{160, 48}, {96, 32}, {333, 7}, {1, 100}, {480, 9}, {1000, 3}};
static const int k_mapped[][2] = {{1, 1}, {1, 5}, {2, 3}, {3, 2}, {4, 3}, {7, 5}, {33, 3}, {61, 4}, {62, 3}, {63, 2}, {64, 1}, {65, 2}, {67, 13}, {1, 130}, {2, 70}, {160, 48}, {480, 9}};

typedef unsigned kind_held; /* a lane's pixel */
typedef struct
{
    unsigned first, last; /* the pixels of the word's first and last byte */
} kind_seen;

#include "ansi_text_check.h"

static char *emitter_text(int width, int rows, const unsigned char *rgb, size_t *size)
{
    trt_emitter *e = NULL;
    if (trt_emitter_create(width, rows, &e) != TRT_HOST_OK || trt_emitter_patch_rgb8(e, rgb) != TRT_HOST_OK)
    {
        fprintf(stderr, "ansi_check: no emitter for %d x %d\n", width, rows);
        exit(2);
    }
    *size = trt_emitter_size(e);
    char *text = (char *)malloc(*size);
    memcpy(text, trt_emitter_buffer(e), *size);
    trt_emitter_destroy(e);
    return text;
}

static unsigned kind_position_byte(const trt_text_at *at, int width, int rows, const unsigned char *rgb)
{
    return trt_ansi_byte(at, rows, at->r >= 0 && at->row < rows ? packed(rgb, trt_text_cell(at, width)) : 0xABCDEFu);
}

static kind_held kind_hold(const trt_text_at *from, int lane, int width, int rows, unsigned width_magic, const unsigned char *rgb)
{
    const long long pixels = (long long)width * rows, p0 = trt_text_cell(from, width);
    (void)width_magic;
    return p0 + lane < pixels ? packed(rgb, p0 + lane) : 0u;
}

static kind_seen kind_colours(const trt_text_at *at, const trt_text_at *last, const trt_text_at *from, const kind_held *mine, int width, long long *rel_first,
                              long long *rel_last)
{
    const long long p0 = trt_text_cell(from, width);
    *rel_first = trt_text_cell(at, width) - p0, *rel_last = trt_text_cell(last, width) - p0;
    const kind_seen shown = {mine[(int)*rel_first & 63], mine[(int)*rel_last & 63]};
    return shown;
}

static unsigned kind_byte(const trt_text_at *at, int rows, kind_seen shown, unsigned other) { return trt_ansi_byte(at, rows, other ? shown.last : shown.first); }

static void kind_constants(void)
{
    if (trt_ansi_text_bytes(0, 5) || trt_ansi_text_bytes(5, 0) || trt_ansi_text_bytes(-1, -1) || trt_ansi_text_bytes(160, 48) != 192057)
        FAIL("trt_ansi_text_bytes of an empty screen, or of 160 x 48");
}
