/*
 * trt_ansi256.h -- the format of a frame's terminal text in the xterm 256-COLOUR PALETTE (host + device, plain C).
 *
 * The text of trt_ansi.h needs 24-bit SGR colour.  This one paints the same two spaces a pixel on a background colour of the fixed
 * part of the xterm palette (trt_xterm256.h: entries 16..255, nearest in RGB bytes, no dithering), for terminals that have only that.
 * The reference has no such emitter; the format is the project's own.  For a screen of `width` x `rows` owned rows, in order,
 *
 *      "\033[0;0H"                                     6 bytes, the home prefix (reset_str, TRT.c:1102)
 *      per owned row:  width cells "\033[48;5;NNNm  "  13 bytes each
 *                      "\033[0m\n"                     5 bytes
 *
 * NNN is the palette index of the pixel's emitter bytes, three zero-padded digits as byte_to_digits makes them (TRT.c:1134-1139).
 * No NUL follows: 6 + (13 width + 5) rows bytes.  trt_emitter_ansi256_rgb8 (csrc/host/trt_emit.c) is the sequential statement.  In
 * trt_text_map.h's terms: cells of 13 bytes, five end bytes per row (bytes 13..17 of the row's last cell), a text row per owned row,
 * no NULs.  That header maps a position of the text to its cell and says which lane of which wave stores which bytes; this one says
 * what stands there.  The device pass (trt_ansi256.hpp) and the host check (tests/ansi256_check.c) compile both.
 *
 * Words per lane.  Lane l of a wave holds cell C0 + l, so a wave's span may touch at most 64 cells (TRT_TEXT_SPAN_CELLS): with cells
 * of 13 bytes that allows three words per lane (768 bytes, 60 cells) and not four (1024 bytes, 80 cells).  Three it is, the most there
 * can be: 60 of 64 lanes then have a pixel to sum, and the once-per-wave work (trt_text_locate's division) is spread over the most
 * bytes.  A head of at most 3 bytes lies in the home prefix (3 < 6), a tail of at most 3 in the last row's five constant end bytes.
 *
 * Which colour a word needs.  The digits of a cell stand at 7..9.  A word that begins in a cell at byte 10 or later reaches, behind
 * it, at most bytes 0..2 of the next cell (through a row's end bytes: of the next row's first cell), and the prefix ends in front of
 * cell 0's byte 0: every digit of a word belongs to the cell of its FIRST byte, and a word is formatted from that one cell's index.
 * What a lane keeps and what the cross-lane read carries is that index, 8 bits, not the colour.
 */
#ifndef TRT_ANSI256_H
#define TRT_ANSI256_H

#include "trt_text_map.h"
#include "trt_xterm256.h"

#define TRT_ANSI256_HD TRT_TEXT_HD

#define TRT_ANSI256_HOME TRT_TEXT_HOME
#define TRT_ANSI256_CELL 13 /* strlen("\033[48;5;000m  ") */
#define TRT_ANSI256_END 5   /* strlen("\033[0m\n") */
#define TRT_ANSI256_NULS 0
#define TRT_ANSI256_WAVE_WORDS 192 /* 3 words per lane */
#define TRT_ANSI256_SPAN (4 * TRT_ANSI256_WAVE_WORDS)
#define TRT_ANSI256_SPAN_CELLS TRT_TEXT_SPAN_CELLS(TRT_ANSI256_CELL, TRT_ANSI256_WAVE_WORDS) /* 60: a wave's cells fit its lanes */

#if TRT_ANSI256_SPAN_CELLS > 64
#error "a wave's cells must fit its 64 lanes"
#endif

/* row: the owned row, `rows` behind the text (a word no lane stores); c in 13..17: the row's end bytes */
typedef trt_text_at trt_ansi256_at;

TRT_ANSI256_HD trt_text_kind trt_ansi256_kind(void)
{
    const trt_text_kind kind = {TRT_ANSI256_CELL, TRT_ANSI256_END, TRT_ANSI256_WAVE_WORDS, TRT_ANSI256_NULS};
    return kind;
}

TRT_ANSI256_HD long long trt_ansi256_text_rows(long long rows) { return rows; }

/* length of the text; 0 for a screen that has none */
TRT_ANSI256_HD unsigned long long trt_ansi256_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0)
        return 0;
    return (unsigned long long)TRT_ANSI256_HOME + (unsigned long long)trt_text_row_bytes(trt_ansi256_kind(), width) * (unsigned long long)rows;
}

/* byte c < 18 of a cell (13..17: the end bytes behind a row's last cell) whose pixel has the palette index `index` */
TRT_ANSI256_HD unsigned trt_ansi256_cell_byte(int c, unsigned index)
{
    const unsigned long long k0 = TRT_TEXT_PACK8(0x1b, '[', '4', '8', ';', '5', ';', '0'), k1 = TRT_TEXT_PACK8('0', '0', 'm', ' ', ' ', 0x1b, '[', '0'),
                             k2 = TRT_TEXT_PACK8('m', '\n', 0, 0, 0, 0, 0, 0);
    const unsigned long long k = c < 8 ? k0 : c < 16 ? k1 : k2;
    const unsigned place = (unsigned)(c - 7); /* digits at 7..9 */
    const unsigned digit = place == 0 ? index / 100u : place == 1 ? (index / 10u) % 10u : index % 10u;
    return ((unsigned)(k >> ((c & 7) * 8)) & 0xffu) + (place < 3u ? digit : 0u);
}

/* what stands at *at inside the text, `index` being the palette index of pixel trt_text_cell(at) */
TRT_ANSI256_HD unsigned trt_ansi256_byte(const trt_ansi256_at *at, unsigned index)
{
    const unsigned home = (unsigned)(TRT_TEXT_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0) >> (((at->r + TRT_ANSI256_HOME) & 7) * 8)) & 0xffu;
    return at->r < 0 ? home : trt_ansi256_cell_byte(at->c & 31, index);
}

/* the value of a byte that a lane of wave 0 stores by itself (trt_text_lone_byte) in a text of `bytes` bytes: the head is in the home
 * prefix, the tail in the last row's end bytes (a text is at least 24 bytes long) */
TRT_ANSI256_HD unsigned trt_ansi256_lone_value(long long position, unsigned long long bytes)
{
    const trt_ansi256_at at = {0, position - TRT_ANSI256_HOME, 0, 0};
    return position < TRT_ANSI256_HOME ? trt_ansi256_byte(&at, 0u)
                                       : trt_ansi256_cell_byte(TRT_ANSI256_CELL + TRT_ANSI256_END - (int)((long long)bytes - position), 0u);
}

#endif /* TRT_ANSI256_H */
