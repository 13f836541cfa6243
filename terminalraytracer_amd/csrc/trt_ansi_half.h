/*
 * trt_ansi_half.h -- the format of a frame's HALF-BLOCK terminal text (host + device, plain C).
 *
 * The text of trt_ansi.h paints a pixel as two spaces on a background colour: two columns and a whole line.  This one paints TWO
 * pixels per character cell with the upper-half-block glyph U+2580: the foreground colour fills the upper half of the cell, the
 * background colour the lower half, so one column and half a line make a (square) pixel.  The reference has no such emitter; the
 * format is the project's own.  For a screen of `width` x `rows` owned rows, T = (rows + 1) / 2 text rows, in order,
 *
 *      "\033[0;0H"                                                              6 bytes, the home prefix (reset_str, TRT.c:1102)
 *      per text row i:  width cells "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm" E2 96 80     39 bytes each
 *                       "\033[0m\n"                                             5 bytes
 *
 * RRR;GGG;BBB are the emitter's bytes of owned row 2 i (the upper pixel), rrr;ggg;bbb those of owned row 2 i + 1 (the lower pixel;
 * 000;000;000 behind the last row of an odd frame), three zero-padded digits each as byte_to_digits makes them (TRT.c:1134-1139).
 * No NUL follows: 6 + (39 width + 5) T bytes.  trt_emitter_half_rgb8 (csrc/host/trt_emit.c) is the sequential statement.  In
 * trt_text_map.h's terms: cells of 39 bytes, five end bytes per row (bytes 39..43 of the row's last cell), T text rows, no NULs, nine
 * words per lane.  That header maps a position of the text to its cell and says which lane of which wave stores which bytes; this
 * one says what stands there and which two pixels a lane holds.  The device pass (trt_ansi_half.hpp) and the host check
 * (tests/ansi_half_check.c) compile both.
 *
 * A span of 2304 bytes touches at most 61 cells (TRT_ANSI_HALF_SPAN_CELLS): lane l holds cell C0 + l, C0 the cell of the wave's first
 * byte, and 61 of 64 lanes have two pixels to sum.
 *
 * Which colour a word needs.  A cell is longer than a word, so a word shows at most two cells.  The digits of a cell stand at 7..17
 * (upper pixel) and 24..34 (lower pixel): bytes 35..43 of a cell and bytes 0..6 of the next hold none, so a word that leaves its
 * first byte's cell shows no digit of either, and the upper and lower digits of one cell are 6 bytes apart, more than a word is
 * long.  Every digit of a word therefore belongs to the cell of its FIRST byte: a word is formatted from that one cell's two
 * colours.
 */
#ifndef TRT_ANSI_HALF_H
#define TRT_ANSI_HALF_H

#include "trt_text_map.h"

#define TRT_ANSI_HALF_HD TRT_TEXT_HD
#define TRT_ANSI_HALF_PACK8 TRT_TEXT_PACK8

#define TRT_ANSI_HALF_HOME TRT_TEXT_HOME
#define TRT_ANSI_HALF_CELL 39 /* strlen("\033[38;2;000;000;000;48;2;000;000;000m") + the glyph's three bytes */
#define TRT_ANSI_HALF_END 5   /* strlen("\033[0m\n") */
#define TRT_ANSI_HALF_NULS 0
#define TRT_ANSI_HALF_WAVE_WORDS 576 /* 9 words per lane */
#define TRT_ANSI_HALF_SPAN (4 * TRT_ANSI_HALF_WAVE_WORDS)
#define TRT_ANSI_HALF_SPAN_CELLS TRT_TEXT_SPAN_CELLS(TRT_ANSI_HALF_CELL, TRT_ANSI_HALF_WAVE_WORDS) /* 61: a wave's cells fit its lanes */

/* row: the text row, T behind the text (a word no lane stores); c in 39..43: the row's end bytes */
typedef trt_text_at trt_ansi_half_at;

TRT_ANSI_HALF_HD trt_text_kind trt_ansi_half_kind(void)
{
    const trt_text_kind kind = {TRT_ANSI_HALF_CELL, TRT_ANSI_HALF_END, TRT_ANSI_HALF_WAVE_WORDS, TRT_ANSI_HALF_NULS};
    return kind;
}

TRT_ANSI_HALF_HD long long trt_ansi_half_text_rows(long long rows) { return (rows + 1) / 2; }

/* length of the text; 0 for a screen that has none */
TRT_ANSI_HALF_HD unsigned long long trt_ansi_half_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0)
        return 0;
    return (unsigned long long)TRT_ANSI_HALF_HOME +
           (unsigned long long)trt_text_row_bytes(trt_ansi_half_kind(), width) * (unsigned long long)trt_ansi_half_text_rows(rows);
}

/* for the width (trt_ansi_half_lane_cell: x < 128 where it is used) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_width_magic(int width) { return trt_text_magic((unsigned long long)width); }

/* byte c < 44 of a cell (39..43: the end bytes behind a row's last cell) whose upper pixel is upper = r | g << 8 | b << 16 and whose
 * lower pixel is lower */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_cell_byte(int c, unsigned upper, unsigned lower)
{
    const unsigned long long k0 = TRT_ANSI_HALF_PACK8(0x1b, '[', '3', '8', ';', '2', ';', '0'), k1 = TRT_ANSI_HALF_PACK8('0', '0', ';', '0', '0', '0', ';', '0'),
                             k2 = TRT_ANSI_HALF_PACK8('0', '0', ';', '4', '8', ';', '2', ';'), k3 = TRT_ANSI_HALF_PACK8('0', '0', '0', ';', '0', '0', '0', ';'),
                             k4 = TRT_ANSI_HALF_PACK8('0', '0', '0', 'm', 0xe2, 0x96, 0x80, 0x1b), k5 = TRT_ANSI_HALF_PACK8('[', '0', 'm', '\n', 0, 0, 0, 0);
    const unsigned long long k = c < 8 ? k0 : c < 16 ? k1 : c < 24 ? k2 : c < 32 ? k3 : c < 40 ? k4 : k5;
    const int low = c >= 24;                        /* digits at 7..9, 11..13, 15..17 and at 24..26, 28..30, 32..34 */
    const unsigned d = (unsigned)(c - (low ? 24 : 7)), rgb = low ? lower : upper;
    const unsigned v = (rgb >> (((d >> 2) & 3u) * 8)) & 0xffu, place = d & 3u;
    const unsigned digit = place == 0 ? v / 100u : place == 1 ? (v / 10u) % 10u : v % 10u;
    return ((unsigned)(k >> ((c & 7) * 8)) & 0xffu) + (d < 11u && place != 3u ? digit : 0u);
}

/* what stands at *at inside the text, upper and lower being the pixels of cell trt_text_cell(at) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_byte(const trt_ansi_half_at *at, unsigned upper, unsigned lower)
{
    const unsigned home = (unsigned)(TRT_ANSI_HALF_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0) >> (((at->r + TRT_ANSI_HALF_HOME) & 7) * 8)) & 0xffu;
    return at->r < 0 ? home : trt_ansi_half_cell_byte(at->c & 63, upper, lower);
}

/* The cell lane `lane` < 64 holds in a wave whose first byte is at *from: text row and column of cell trt_text_cell(from) + lane.
 * from->col + lane < width + 64: no or one row further on where rows are wide, a multiply-high where they are narrow (x < 128; the
 * magic of width 1 would be 2^32, which 32 bits do not hold: there the quotient is x itself). */
TRT_ANSI_HALF_HD void trt_ansi_half_lane_cell(const trt_ansi_half_at *from, int lane, int width, unsigned width_magic, long long *trow, int *col)
{
    const unsigned x = (unsigned)from->col + (unsigned)lane;
    const unsigned q = width >= 64 ? (unsigned)(x >= (unsigned)width) : width == 1 ? x : (unsigned)(((unsigned long long)x * width_magic) >> 32);
    *trow = from->row + q;
    *col = (int)(x - q * (unsigned)width);
}

/* the value of a byte that a lane of wave 0 stores by itself (trt_text_lone_byte) in a text of `bytes` bytes: the head is in the home
 * prefix, the tail in the last row's end bytes (a text is at least 50 bytes long) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_lone_value(long long position, unsigned long long bytes)
{
    const trt_ansi_half_at at = {0, position - TRT_ANSI_HALF_HOME, 0, 0};
    return position < TRT_ANSI_HALF_HOME ? trt_ansi_half_byte(&at, 0, 0)
                                         : trt_ansi_half_cell_byte(TRT_ANSI_HALF_CELL + TRT_ANSI_HALF_END - (int)((long long)bytes - position), 0, 0);
}

#endif /* TRT_ANSI_HALF_H */
