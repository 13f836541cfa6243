/*
 * trt_ansi_delta_half.h -- the DELTA text of a frame in HALF-BLOCK cells: what a terminal that shows frame `shown` as the text of
 * trt_ansi_half.h must be sent to show frame `next` (host + device, plain C).  The reference has no such emitter; this header is the
 * format's one specification in code, and trt_emitter_delta_half_rgb8 (csrc/host/trt_emit.c) its sequential statement.
 *
 * Two frames of RGB8 bytes, rows x width x 3.  The cells are those of trt_ansi_half.h: T = (rows + 1) / 2 text rows of `width` cells,
 * cell (t, c) with the UPPER pixel of owned row 2 t and the LOWER pixel of owned row 2 t + 1; behind an odd frame's last row the lower
 * pixel is 000;000;000 in both frames and is never read from memory.  A cell is CHANGED when either of its pixels differs between the
 * frames.  A RUN is a maximal sequence of consecutive changed cells of one text row.  The text is the concatenation, text rows
 * ascending, cells left to right, of the RECORDS of the changed cells; an unchanged cell has none.  A record is, in this order,
 *
 *   1. if the cell starts a run:  "\033[RRRRR;CCCCCH"          14 bytes, RRRRR = t + 1, CCCCC = c + 1 (a cell is ONE column wide)
 *   2. the colours, against those of the cell to the left, which a run has just painted:
 *        it starts a run, or BOTH new colours differ from the left neighbour's new colours:
 *                                 "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm"   36 bytes, bytes 0..35 of the half-block cell
 *        only the upper differs:  "\033[38;2;RRR;GGG;BBBm"     19 bytes
 *        only the lower differs:  "\033[48;2;rrr;ggg;bbbm"     19 bytes
 *        neither differs:         nothing
 *   3. always:                    the glyph E2 96 80           3 bytes
 *   4. if it ends a run:          "\033[0m"                    4 bytes
 *
 * so a record is 3, 7, 22, 26, 39, 43, 53 or 57 bytes long -- a function of the cell and its two neighbours.  No prefix, no newline,
 * no NUL; equal frames give no text.
 *
 * The bound, by the argument of trt_ansi_delta.h.  A run of L cells costs at most 14 + 36 L + 3 L + 4 = 18 + 39 L bytes.  A row's
 * runs are separated by at least one unchanged cell, so k runs hold at most width - (k - 1) cells: at most
 * 18 k + 39 (width - k + 1) = 39 width + 39 - 21 k bytes, largest at k = 1: 39 width + 18 per text row, T (39 width + 18) per text.
 * A frame whose every cell changed, with both colours different from the left neighbour's everywhere, reaches it.  It exceeds the
 * whole half-block text 6 + T (39 width + 5) for every T >= 1 (13 T > 6); the capacity is written as the larger of the two all the
 * same, as trt_ansi_delta_capacity is.
 *
 * The limits.  Five decimal digits for t + 1 and for c + 1: width <= 99999, T <= 99999 (rows <= 199998).
 *
 * How the device writes it: the scheme of trt_ansi_delta.h -- cells numbered row-major over the TEXT rows, tiles of TRT_DELTA_TILE
 * cells, TRT_DELTA_LANE_CELLS consecutive cells per lane, lengths per cell, sums per tile (at most 1024 x 57 = 58 368 bytes: 32 bits),
 * an exclusive scan of the tiles' sums, a scan inside the tile.  The LANE'S WALK is here, trt_delta_half_lane_cells: which bytes of
 * the two frames lane `thread` of tile `tile` loads -- never the pixel row behind an odd frame -- its cells' text rows and columns
 * across the end of a row, its records' lengths; trt_delta_half_lane_byte gives the bytes.  The kernels of trt_ansi_delta.hpp and
 * tests/ansi_delta_half_check.c call the two as they call those of trt_ansi_delta.h.
 */
#ifndef TRT_ANSI_DELTA_HALF_H
#define TRT_ANSI_DELTA_HALF_H

#include "trt_ansi_delta.h"
#include "trt_ansi_half.h"

#define TRT_DELTA_HALF_BOTH 36   /* strlen("\033[38;2;000;000;000;48;2;000;000;000m") */
#define TRT_DELTA_HALF_SINGLE 19 /* strlen("\033[38;2;000;000;000m") == strlen("\033[48;2;000;000;000m") */
#define TRT_DELTA_HALF_GLYPH 3
#define TRT_DELTA_HALF_RECORD_MAX (TRT_DELTA_CURSOR + TRT_DELTA_HALF_BOTH + TRT_DELTA_HALF_GLYPH + TRT_DELTA_RESET) /* 57 */
#define TRT_DELTA_HALF_MAX_WIDTH 99999
#define TRT_DELTA_HALF_MAX_TEXT_ROWS 99999

/* the neighbourhood of a cell a record depends on.  changed_left is 0 in column 0, changed_right 0 in the last column; the two same_
 * flags compare the NEW colours with the left neighbour's and mean nothing in column 0 (a run starts there) */
typedef struct
{
    int changed_left, changed, changed_right, same_upper, same_lower;
} trt_delta_half_flags;

TRT_ANSI_HD int trt_delta_half_size_ok(int width, long long rows)
{
    return width > 0 && rows > 0 && width <= TRT_DELTA_HALF_MAX_WIDTH && (rows + 1) / 2 <= TRT_DELTA_HALF_MAX_TEXT_ROWS;
}

/* the most bytes a half-block delta text of width x rows can have; 0 for a screen that has none */
TRT_ANSI_HD unsigned long long trt_delta_half_bound(int width, long long rows)
{
    if (!trt_delta_half_size_ok(width, rows))
        return 0;
    return (unsigned long long)((rows + 1) / 2) * (39ull * (unsigned)width + 18ull);
}

/* room for any text a half-block delta entry writes: a delta or the keyframe, the whole half-block text */
TRT_ANSI_HD unsigned long long trt_delta_half_capacity(int width, long long rows)
{
    if (!trt_delta_half_size_ok(width, rows))
        return 0;
    const unsigned long long whole = trt_ansi_half_text_bytes(width, rows), bound = trt_delta_half_bound(width, rows);
    return whole > bound ? whole : bound;
}

TRT_ANSI_HD int trt_delta_half_starts(const trt_delta_half_flags *f) { return f->changed && !f->changed_left; }
TRT_ANSI_HD int trt_delta_half_ends(const trt_delta_half_flags *f) { return f->changed && !f->changed_right; }
/* which colours the record sets: the upper one, the lower one */
TRT_ANSI_HD int trt_delta_half_upper(const trt_delta_half_flags *f) { return f->changed && (!f->changed_left || !f->same_upper); }
TRT_ANSI_HD int trt_delta_half_lower(const trt_delta_half_flags *f) { return f->changed && (!f->changed_left || !f->same_lower); }

TRT_ANSI_HD unsigned trt_delta_half_colour_bytes(const trt_delta_half_flags *f)
{
    const int upper = trt_delta_half_upper(f), lower = trt_delta_half_lower(f);
    return upper && lower ? TRT_DELTA_HALF_BOTH : upper || lower ? TRT_DELTA_HALF_SINGLE : 0;
}

/* length of the cell's record: 0 (unchanged), 3, 7, 22, 26, 39, 43, 53 or 57 */
TRT_ANSI_HD unsigned trt_delta_half_record_bytes(const trt_delta_half_flags *f)
{
    if (!f->changed)
        return 0;
    return (trt_delta_half_starts(f) ? TRT_DELTA_CURSOR : 0) + trt_delta_half_colour_bytes(f) + TRT_DELTA_HALF_GLYPH + (trt_delta_half_ends(f) ? TRT_DELTA_RESET : 0);
}

/* byte k < 14 of the cursor address of cell (t, c) */
TRT_ANSI_HD unsigned trt_delta_half_cursor_byte(unsigned k, int t, int c)
{
    const unsigned long long k0 = TRT_ANSI_PACK8(0x1b, '[', '0', '0', '0', '0', '0', ';'), k1 = TRT_ANSI_PACK8('0', '0', '0', '0', '0', 'H', 0, 0);
    const unsigned d = k < 8 ? k - 2 : k - 8; /* digits at 2..6 and 8..12, most significant first */
    const unsigned v = k < 8 ? (unsigned)t + 1u : (unsigned)c + 1u;
    const unsigned digit = d == 0 ? v / 10000u : d == 1 ? (v / 1000u) % 10u : d == 2 ? (v / 100u) % 10u : d == 3 ? (v / 10u) % 10u : v % 10u;
    return ((unsigned)((k < 8 ? k0 : k1) >> ((k & 7) * 8)) & 0xffu) + (d < 5u ? digit : 0u);
}

/* byte k < trt_delta_half_record_bytes(f) of the record of cell (t, c) whose new pixels are upper and lower = r | g << 8 | b << 16.
 * Behind the cursor a record is a piece of the half-block cell's 39 bytes and of the row's end bytes behind them (trt_ansi_half_cell_byte,
 * 0..42): both colours are its bytes 0..35; the upper colour alone its bytes 0..17 and the 'm' at 35; the lower colour alone its bytes
 * 0, 1 and 19..35 ("\033[" in front of "48;2;"); the glyph its bytes 36..38, the reset 39..42. */
TRT_ANSI_HD unsigned trt_delta_half_record_byte(unsigned k, int t, int c, unsigned upper, unsigned lower, const trt_delta_half_flags *f)
{
    const unsigned cursor = trt_delta_half_starts(f) ? TRT_DELTA_CURSOR : 0;
    if (k < cursor)
        return trt_delta_half_cursor_byte(k, t, c);
    k -= cursor;
    const unsigned colour = trt_delta_half_colour_bytes(f);
    unsigned at;
    if (k >= colour)
        at = TRT_DELTA_HALF_BOTH + (k - colour);
    else if (colour == TRT_DELTA_HALF_BOTH)
        at = k;
    else if (trt_delta_half_upper(f))
        at = k < TRT_DELTA_HALF_SINGLE - 1 ? k : TRT_DELTA_HALF_BOTH - 1;
    else
        at = k < 2 ? k : k + (TRT_DELTA_HALF_BOTH - TRT_DELTA_HALF_SINGLE);
    return trt_ansi_half_cell_byte((int)at, upper, lower);
}

/* a lane's cells: their new colours, what their records depend on, the records' lengths and their sum, and where the cells lie */
typedef struct
{
    unsigned upper[TRT_DELTA_LANE_CELLS], lower[TRT_DELTA_LANE_CELLS], bytes[TRT_DELTA_LANE_CELLS];
    trt_delta_half_flags flags[TRT_DELTA_LANE_CELLS];
    int trow[TRT_DELTA_LANE_CELLS], col[TRT_DELTA_LANE_CELLS];
    unsigned total;
} trt_delta_half_lane;

/* The cells tile * TRT_DELTA_TILE + TRT_DELTA_LANE_CELLS * thread + j of a frame of width x rows pixels, (rows + 1) / 2 text rows; those
 * behind the frame have no record and are not loaded.  One 64-bit division per workgroup (where the tile starts), one 32-bit division
 * per lane.  Cell (t, col) has its upper pixel at pixel 2 t width + col of a frame and its lower one `width` pixels on, which exists,
 * and is loaded, when 2 t + 1 < rows. */
TRT_ANSI_HD trt_delta_half_lane trt_delta_half_lane_cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile,
                                                          unsigned thread)
{
    const unsigned trows = ((unsigned)rows + 1u) / 2u;
    const unsigned long long tile_first = tile * TRT_DELTA_TILE;
    const unsigned long long tile_row = tile_first / (unsigned)width;
    const unsigned x = (unsigned)(tile_first - tile_row * (unsigned)width) + TRT_DELTA_LANE_CELLS * thread; /* < 99 999 + 1024 */
    const unsigned q = x / (unsigned)width;
    /* the lane's cells and a neighbour either side, [j + 1] the j-th: cell -1 only matters inside a row, so it is read only there */
    unsigned long long t = tile_row + q;
    int col = (int)(x - q * (unsigned)width) - 1;
    unsigned up[TRT_DELTA_LANE_CELLS + 2], low[TRT_DELTA_LANE_CELLS + 2];
    int changed[TRT_DELTA_LANE_CELLS + 2];
    trt_delta_half_lane c;
    TRT_DELTA_UNROLL
    for (int j = -1; j <= TRT_DELTA_LANE_CELLS; j++)
    {
        const int there = col >= 0 && t < trows;
        const int has_lower = there && 2 * t + 1 < (unsigned long long)(unsigned)rows;
        const unsigned long long p = 2 * t * (unsigned)width + (unsigned)col; /* used only where `there` */
        up[j + 1] = there ? trt_delta_rgb(next, p) : 0u;
        low[j + 1] = has_lower ? trt_delta_rgb(next, p + (unsigned)width) : 0u;
        changed[j + 1] = there && (up[j + 1] != trt_delta_rgb(shown, p) || (has_lower && low[j + 1] != trt_delta_rgb(shown, p + (unsigned)width)));
        if (j >= 0 && j < TRT_DELTA_LANE_CELLS)
        {
            c.trow[j] = (int)t;
            c.col[j] = col;
        }
        if (++col == width)
            col = 0, t++;
    }
    c.total = 0;
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.upper[j] = up[j + 1];
        c.lower[j] = low[j + 1];
        c.flags[j].changed = changed[j + 1];
        c.flags[j].changed_left = c.col[j] > 0 && changed[j];
        c.flags[j].changed_right = c.col[j] + 1 < width && changed[j + 2];
        c.flags[j].same_upper = up[j + 1] == up[j];
        c.flags[j].same_lower = low[j + 1] == low[j];
        c.bytes[j] = trt_delta_half_record_bytes(&c.flags[j]);
        c.total += c.bytes[j];
    }
    return c;
}

/* byte k < c->bytes[j] of the record of the lane's j-th cell */
TRT_ANSI_HD unsigned trt_delta_half_lane_byte(const trt_delta_half_lane *c, int j, unsigned k)
{
    return trt_delta_half_record_byte(k, c->trow[j], c->col[j], c->upper[j], c->lower[j], &c->flags[j]);
}

#endif /* TRT_ANSI_DELTA_HALF_H */
