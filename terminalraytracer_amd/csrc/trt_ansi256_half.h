/*
 * trt_ansi256_half.h -- the format of a frame's HALF-BLOCK terminal text in the xterm 256-COLOUR PALETTE (host + device, plain C).
 *
 * The text of trt_ansi_half.h -- two pixels per character cell, the upper one as the foreground and the lower one as the background
 * colour of the upper-half-block glyph U+2580 -- for terminals without 24-bit SGR colour: both colours are entries of the fixed part
 * of the xterm palette (trt_xterm256.h: entries 16..255, nearest in RGB bytes, no dithering).  The format is the project's own.  For a
 * screen of `width` x `rows` owned rows, T = (rows + 1) / 2 text rows, in order,
 *
 *      "\033[0;0H"                                                  6 bytes, the home prefix (reset_str, TRT.c:1102)
 *      per text row t:  width cells "\033[38;5;UUU;48;5;LLLm" E2 96 80     23 bytes each
 *                       "\033[0m\n"                                 5 bytes
 *
 * UUU is the palette index of the emitter's bytes of owned row 2 t (the upper pixel), LLL that of owned row 2 t + 1 (the lower pixel;
 * 016, the palette's black, behind the last row of an odd frame), three zero-padded digits each as byte_to_digits makes them
 * (TRT.c:1134-1139).  No NUL follows: 6 + (23 width + 5) T bytes.  trt_emitter_ansi256_half_rgb8 (csrc/host/trt_emit.c) is the
 * sequential statement.  In trt_text_map.h's terms: cells of 23 bytes, five end bytes per row (bytes 23..27 of the row's last cell),
 * T text rows, no NULs.  That header maps a position of the text to its cell and says which lane of which wave stores which bytes;
 * this one says what stands there and which two pixels a lane holds.  The device pass (trt_ansi256.hpp) and the host check
 * (tests/ansi256_half_check.c) compile both.
 *
 * Words per lane.  Lane l of a wave holds cell C0 + l, so a wave's span may touch at most 64 cells (TRT_TEXT_SPAN_CELLS): with cells
 * of 23 bytes that allows five words per lane (1280 bytes, 57 cells) and not six (1536 bytes, 68 cells).  Five it is, the most there
 * can be: 57 of 64 lanes then have two pixels to sum -- four words would leave 46 -- and the once-per-wave work is spread over the
 * most bytes.  A head of at most 3 bytes lies in the home prefix (3 < 6), a tail of at most 3 in the last row's five constant end
 * bytes.
 *
 * Which colours a word needs.  The digits of a cell stand at 7..9 (upper pixel) and 16..18 (lower pixel).  A word that begins in a
 * cell at byte 19 or later reaches, behind it, at most bytes 0..2 of the next cell (through a row's end bytes: of the next row's
 * first cell), and the prefix ends in front of cell 0's byte 0: every digit of a word belongs to the cell of its FIRST byte, and a
 * word is formatted from that one cell's two indices.  What a lane keeps and what the cross-lane read carries is those two indices,
 * 16 bits in one register, not the colours.
 */
#ifndef TRT_ANSI256_HALF_H
#define TRT_ANSI256_HALF_H

#include "trt_text_map.h"
#include "trt_xterm256.h"

#define TRT_ANSI256_HALF_HD TRT_TEXT_HD

#define TRT_ANSI256_HALF_HOME TRT_TEXT_HOME
#define TRT_ANSI256_HALF_CELL 23 /* strlen("\033[38;5;000;48;5;000m") + the glyph's three bytes */
#define TRT_ANSI256_HALF_END 5   /* strlen("\033[0m\n") */
#define TRT_ANSI256_HALF_NULS 0
#define TRT_ANSI256_HALF_WAVE_WORDS 320 /* 5 words per lane */
#define TRT_ANSI256_HALF_SPAN (4 * TRT_ANSI256_HALF_WAVE_WORDS)
#define TRT_ANSI256_HALF_SPAN_CELLS TRT_TEXT_SPAN_CELLS(TRT_ANSI256_HALF_CELL, TRT_ANSI256_HALF_WAVE_WORDS) /* 57: a wave's cells fit its lanes */

#if TRT_ANSI256_HALF_SPAN_CELLS > 64
#error "a wave's cells must fit its 64 lanes"
#endif

/* row: the text row, T behind the text (a word no lane stores); c in 23..27: the row's end bytes */
typedef trt_text_at trt_ansi256_half_at;

TRT_ANSI256_HALF_HD trt_text_kind trt_ansi256_half_kind(void)
{
    const trt_text_kind kind = {TRT_ANSI256_HALF_CELL, TRT_ANSI256_HALF_END, TRT_ANSI256_HALF_WAVE_WORDS, TRT_ANSI256_HALF_NULS};
    return kind;
}

TRT_ANSI256_HALF_HD long long trt_ansi256_half_text_rows(long long rows) { return (rows + 1) / 2; }

/* length of the text; 0 for a screen that has none */
TRT_ANSI256_HALF_HD unsigned long long trt_ansi256_half_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0)
        return 0;
    return (unsigned long long)TRT_ANSI256_HALF_HOME +
           (unsigned long long)trt_text_row_bytes(trt_ansi256_half_kind(), width) * (unsigned long long)trt_ansi256_half_text_rows(rows);
}

/* for the width (trt_ansi256_half_lane_cell: x < 128 where it is used) */
TRT_ANSI256_HALF_HD unsigned trt_ansi256_half_width_magic(int width) { return trt_text_magic((unsigned long long)width); }

/* a cell's two palette indices as a lane holds them */
TRT_ANSI256_HALF_HD unsigned trt_ansi256_half_pair(unsigned upper, unsigned lower) { return upper | lower << 8; }

/* byte c < 28 of a cell (23..27: the end bytes behind a row's last cell) whose indices are pair = upper | lower << 8 */
TRT_ANSI256_HALF_HD unsigned trt_ansi256_half_cell_byte(int c, unsigned pair)
{
    const unsigned long long k0 = TRT_TEXT_PACK8(0x1b, '[', '3', '8', ';', '5', ';', '0'), k1 = TRT_TEXT_PACK8('0', '0', ';', '4', '8', ';', '5', ';'),
                             k2 = TRT_TEXT_PACK8('0', '0', '0', 'm', 0xe2, 0x96, 0x80, 0x1b), k3 = TRT_TEXT_PACK8('[', '0', 'm', '\n', 0, 0, 0, 0);
    const unsigned long long k = c < 8 ? k0 : c < 16 ? k1 : c < 24 ? k2 : k3;
    const int low = c >= 16; /* digits at 7..9 and at 16..18 */
    const unsigned place = (unsigned)(c - (low ? 16 : 7)), index = (low ? pair >> 8 : pair) & 0xffu;
    const unsigned digit = place == 0 ? index / 100u : place == 1 ? (index / 10u) % 10u : index % 10u;
    return ((unsigned)(k >> ((c & 7) * 8)) & 0xffu) + (place < 3u ? digit : 0u);
}

/* what stands at *at inside the text, `pair` being the indices of cell trt_text_cell(at) */
TRT_ANSI256_HALF_HD unsigned trt_ansi256_half_byte(const trt_ansi256_half_at *at, unsigned pair)
{
    const unsigned home = (unsigned)(TRT_TEXT_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0) >> (((at->r + TRT_ANSI256_HALF_HOME) & 7) * 8)) & 0xffu;
    return at->r < 0 ? home : trt_ansi256_half_cell_byte(at->c & 31, pair);
}

/* The cell lane `lane` < 64 holds in a wave whose first byte is at *from: text row and column of cell trt_text_cell(from) + lane.
 * from->col + lane < width + 64: no or one row further on where rows are wide, a multiply-high where they are narrow (x < 128; the
 * magic of width 1 would be 2^32, which 32 bits do not hold: there the quotient is x itself). */
TRT_ANSI256_HALF_HD void trt_ansi256_half_lane_cell(const trt_ansi256_half_at *from, int lane, int width, unsigned width_magic, long long *trow, int *col)
{
    const unsigned x = (unsigned)from->col + (unsigned)lane;
    const unsigned q = width >= 64 ? (unsigned)(x >= (unsigned)width) : width == 1 ? x : (unsigned)(((unsigned long long)x * width_magic) >> 32);
    *trow = from->row + q;
    *col = (int)(x - q * (unsigned)width);
}

/* the value of a byte that a lane of wave 0 stores by itself (trt_text_lone_byte) in a text of `bytes` bytes: the head is in the home
 * prefix, the tail in the last row's end bytes (a text is at least 34 bytes long) */
TRT_ANSI256_HALF_HD unsigned trt_ansi256_half_lone_value(long long position, unsigned long long bytes)
{
    const trt_ansi256_half_at at = {0, position - TRT_ANSI256_HALF_HOME, 0, 0};
    return position < TRT_ANSI256_HALF_HOME
               ? trt_ansi256_half_byte(&at, 0u)
               : trt_ansi256_half_cell_byte(TRT_ANSI256_HALF_CELL + TRT_ANSI256_HALF_END - (int)((long long)bytes - position), 0u);
}

#endif /* TRT_ANSI256_HALF_H */
