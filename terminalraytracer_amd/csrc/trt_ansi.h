/*
 * trt_ansi.h -- the format of a frame's terminal text (host + device, plain C).
 *
 * buffered_draw_screen (TRT.c:1142-1172) patches nine decimal digits per pixel into a pre-formatted buffer and writes all of it:
 * for a frame of `width` x `rows` owned rows, in order,
 *
 *      "\033[0;0H"                                               6 bytes, the home prefix
 *      per row:  width cells "\033[48;2;RRR;GGG;BBBm  \033[0m"  25 bytes each, then '\n'
 *      three NUL bytes                                           (the reference writes sizeof(screenbuffer), TRT.c:1104)
 *
 * 8 + (25 width + 1) rows + 1 bytes: what trt_emitter_create / trt_emitter_patch_rgb8 (csrc/host/trt_emit.c) leave in the emitter's
 * buffer.  In trt_text_map.h's terms: cells of 25 bytes, one end byte per row (the newline: byte 25 of the row's last cell), a text
 * row per owned row, three NULs, six words per lane.  That header maps a position of the text to its cell and says which lane of
 * which wave stores which bytes; this one says what stands there.  The device pass that writes the text (trt_ansi.hpp) and the host
 * check (tests/ansi_check.c) compile both.
 *
 * A span of 1536 bytes touches at most 63 cells (TRT_ANSI_SPAN_CELLS): the pixels a wave's words show are P0 .. P0 + 62, P0 the pixel
 * of the wave's first byte, and lane l holds pixel P0 + l.  A cell is longer than a word, so a word shows at most two pixels: that of
 * its first byte and that of its last.
 */
#ifndef TRT_ANSI_H
#define TRT_ANSI_H

#include "trt_text_map.h"

#define TRT_ANSI_HD TRT_TEXT_HD
#define TRT_ANSI_PACK8 TRT_TEXT_PACK8

#define TRT_ANSI_HOME TRT_TEXT_HOME
#define TRT_ANSI_CELL 25 /* strlen(pixel_str), TRT.c:1103 */
#define TRT_ANSI_END 1   /* the newline */
#define TRT_ANSI_NULS 3
#define TRT_ANSI_WAVE_WORDS 384 /* 6 words per lane */
#define TRT_ANSI_SPAN (4 * TRT_ANSI_WAVE_WORDS)
#define TRT_ANSI_SPAN_CELLS TRT_TEXT_SPAN_CELLS(TRT_ANSI_CELL, TRT_ANSI_WAVE_WORDS) /* 63: a wave's pixels fit its lanes */

/* row: the owned row, `rows` in the three NULs (r: which of them); c == 25: the newline */
typedef trt_text_at trt_ansi_at;

TRT_ANSI_HD trt_text_kind trt_ansi_kind(void)
{
    const trt_text_kind kind = {TRT_ANSI_CELL, TRT_ANSI_END, TRT_ANSI_WAVE_WORDS, TRT_ANSI_NULS};
    return kind;
}

TRT_ANSI_HD long long trt_ansi_text_rows(long long rows) { return rows; }

/* length of the text; 0 for a screen that has none */
TRT_ANSI_HD unsigned long long trt_ansi_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0)
        return 0;
    return (unsigned long long)(TRT_ANSI_HOME + 2) + (unsigned long long)trt_text_row_bytes(trt_ansi_kind(), width) * (unsigned long long)rows + 1;
}

/* byte c of the cell of a pixel rgb = r | g << 8 | b << 16: pixel_str with byte_to_digits' digits in it (TRT.c:1134-1139) */
TRT_ANSI_HD unsigned trt_ansi_cell_byte(int c, unsigned rgb)
{
    const unsigned long long k0 = TRT_ANSI_PACK8(0x1b, '[', '4', '8', ';', '2', ';', '0'), k1 = TRT_ANSI_PACK8('0', '0', ';', '0', '0', '0', ';', '0'),
                             k2 = TRT_ANSI_PACK8('0', '0', 'm', ' ', ' ', 0x1b, '[', '0'), k3 = 'm';
    const unsigned long long k = c < 8 ? k0 : c < 16 ? k1 : c < 24 ? k2 : k3;
    const unsigned d = (unsigned)(c - 7); /* digits at 7..9, 11..13, 15..17 */
    const unsigned v = (rgb >> (((d >> 2) & 3u) * 8)) & 0xffu, place = d & 3u;
    const unsigned digit = place == 0 ? v / 100u : place == 1 ? (v / 10u) % 10u : v % 10u;
    return ((unsigned)(k >> ((c & 7) * 8)) & 0xffu) + (d < 11u && place != 3u ? digit : 0u);
}

/* what stands at *at, rgb being the bytes of pixel trt_text_cell(at): 0 in the prefix, width * rows in the NULs, where rgb plays no part */
TRT_ANSI_HD unsigned trt_ansi_byte(const trt_ansi_at *at, long long rows, unsigned rgb)
{
    const unsigned home = (unsigned)(TRT_ANSI_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0) >> (((at->r + TRT_ANSI_HOME) & 7) * 8)) & 0xffu;
    const unsigned cell = at->c == TRT_ANSI_CELL ? (unsigned)'\n' : trt_ansi_cell_byte(at->c & 31, rgb);
    return at->r < 0 ? home : at->row >= rows ? 0u : cell;
}

/* the value of a byte that a lane of wave 0 stores by itself (trt_text_lone_byte): the head is in the home prefix, the tail in the
 * NULs (a text is at least 35 bytes long) */
TRT_ANSI_HD unsigned trt_ansi_lone_value(long long position, unsigned long long bytes)
{
    const trt_ansi_at at = {0, position - TRT_ANSI_HOME, 0, 0};
    (void)bytes;
    return position < TRT_ANSI_HOME ? trt_ansi_byte(&at, 1, 0) : 0u;
}

#endif /* TRT_ANSI_H */
