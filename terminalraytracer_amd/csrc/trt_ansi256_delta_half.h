/*
 * trt_ansi256_delta_half.h -- the DELTA text of a frame in HALF-BLOCK cells in the xterm 256-COLOUR PALETTE: what a terminal that
 * shows frame `shown` as the text of trt_ansi256_half.h must be sent to show frame `next` (host + device, plain C).  The reference has
 * no such emitter; this header is the format's one specification in code, and trt_emitter_delta256_half_rgb8 (csrc/host/trt_emit.c)
 * its sequential statement.
 *
 * Two frames of RGB8 bytes, rows x width x 3.  A pixel's INDEX is trt_xterm256_index_of of its three bytes (trt_xterm256.h).  The
 * cells are those of trt_ansi256_half.h: T = (rows + 1) / 2 text rows of `width` cells, cell (t, c) with the UPPER pixel of owned row
 * 2 t and the LOWER pixel of owned row 2 t + 1; behind an odd frame's last row the lower index is TRT_XTERM256_BLACK (016) in both
 * frames and that row is never read from memory.  A cell is CHANGED when either of its INDICES differs between the frames -- not when
 * a byte does.  A RUN is a maximal sequence of consecutive changed cells of one text row.  The text is the concatenation, text rows
 * ascending, cells left to right, of the RECORDS of the changed cells; an unchanged cell has none.  A record is, in this order,
 *
 *   1. if the cell starts a run:  "\033[RRRRR;CCCCCH"          14 bytes, RRRRR = t + 1, CCCCC = c + 1 (a cell is ONE column wide)
 *   2. the colours, the new INDICES against those of the cell to the left, which a run has just painted:
 *        it starts a run, or BOTH differ from the left neighbour's:
 *                                 "\033[38;5;UUU;48;5;LLLm"    20 bytes, bytes 0..19 of the palette's half-block cell
 *        only the upper differs:  "\033[38;5;UUUm"             11 bytes
 *        only the lower differs:  "\033[48;5;LLLm"             11 bytes
 *        neither differs:         nothing
 *   3. always:                    the glyph E2 96 80           3 bytes
 *   4. if it ends a run:          "\033[0m"                    4 bytes
 *
 * so a record is 3, 7, 14, 18, 23, 27, 37 or 41 bytes long -- a function of the cell and its two neighbours.  No prefix, no newline,
 * no NUL; frames of equal indices give no text.
 *
 * The bound, by the argument of trt_ansi_delta_half.h.  A run of L cells costs at most 14 + 20 L + 3 L + 4 = 18 + 23 L bytes.  A
 * row's runs are separated by at least one unchanged cell, so k runs hold at most width - (k - 1) cells: at most
 * 18 k + 23 (width - k + 1) = 23 width + 23 - 5 k bytes.  A run's fixed cost (18) is BELOW a cell's (23) -- unlike the full cells of
 * trt_ansi256_delta.h -- so one run is worst: 23 width + 18 per text row, T (23 width + 18) per text.  A frame whose every cell
 * changed, with both indices different from the left neighbour's everywhere, reaches it.  It exceeds the whole palette text
 * 6 + T (23 width + 5) for every T >= 1 (13 T > 6); the capacity is written as the larger of the two all the same.
 *
 * The limits.  Five decimal digits for t + 1 and for c + 1: width <= 99999, T <= 99999 (rows <= 199998).
 *
 * How the device writes it: the scheme of trt_ansi_delta.h -- cells numbered row-major over the TEXT rows, tiles of TRT_DELTA_TILE
 * cells, TRT_DELTA_LANE_CELLS consecutive cells per lane, lengths per cell, sums per tile (at most 1024 x 41 = 41 984 bytes: 32 bits),
 * an exclusive scan of the tiles' sums, a scan inside the tile.  The LANE'S WALK is here, trt_delta256_half_lane_cells: which bytes of
 * the two frames lane `thread` of tile `tile` loads and maps to indices -- never the pixel row behind an odd frame; the frames stay
 * RGB8 --, its cells' text rows and columns across the end of a row, its records' lengths; trt_delta256_half_lane_byte gives the
 * bytes.  The kernels of trt_ansi_delta.hpp and tests/ansi256_delta_check.c call the two as they call those of trt_ansi_delta_half.h.
 */
#ifndef TRT_ANSI256_DELTA_HALF_H
#define TRT_ANSI256_DELTA_HALF_H

#include "trt_ansi256_half.h"
#include "trt_ansi_delta_half.h"

#define TRT_DELTA256_HALF_BOTH 20   /* strlen("\033[38;5;000;48;5;000m") */
#define TRT_DELTA256_HALF_SINGLE 11 /* strlen("\033[38;5;000m") == strlen("\033[48;5;000m") */
#define TRT_DELTA256_HALF_RECORD_MAX (TRT_DELTA_CURSOR + TRT_DELTA256_HALF_BOTH + TRT_DELTA_HALF_GLYPH + TRT_DELTA_RESET) /* 41 */
#define TRT_DELTA256_HALF_MAX_WIDTH TRT_DELTA_HALF_MAX_WIDTH
#define TRT_DELTA256_HALF_MAX_TEXT_ROWS TRT_DELTA_HALF_MAX_TEXT_ROWS

TRT_ANSI_HD int trt_delta256_half_size_ok(int width, long long rows)
{
    return width > 0 && rows > 0 && width <= TRT_DELTA256_HALF_MAX_WIDTH && (rows + 1) / 2 <= TRT_DELTA256_HALF_MAX_TEXT_ROWS;
}

/* the most bytes a text row of `width` cells can have: one run */
TRT_ANSI_HD unsigned long long trt_delta256_half_row_bound(int width) { return 23ull * (unsigned)width + 18ull; }

/* the most bytes a half-block palette delta text of width x rows can have; 0 for a screen that has none */
TRT_ANSI_HD unsigned long long trt_delta256_half_bound(int width, long long rows)
{
    if (!trt_delta256_half_size_ok(width, rows))
        return 0;
    return (unsigned long long)((rows + 1) / 2) * trt_delta256_half_row_bound(width);
}

/* room for any text a half-block palette delta entry writes: a delta or the keyframe, the whole half-block palette text */
TRT_ANSI_HD unsigned long long trt_delta256_half_capacity(int width, long long rows)
{
    if (!trt_delta256_half_size_ok(width, rows))
        return 0;
    const unsigned long long whole = trt_ansi256_half_text_bytes(width, rows), bound = trt_delta256_half_bound(width, rows);
    return whole > bound ? whole : bound;
}

/* The neighbourhood of a cell is trt_delta_half_flags, the two same_ flags comparing the NEW INDICES; starts, ends, upper and lower are
 * those of trt_ansi_delta_half.h. */
TRT_ANSI_HD unsigned trt_delta256_half_colour_bytes(const trt_delta_half_flags *f)
{
    const int upper = trt_delta_half_upper(f), lower = trt_delta_half_lower(f);
    return upper && lower ? TRT_DELTA256_HALF_BOTH : upper || lower ? TRT_DELTA256_HALF_SINGLE : 0;
}

/* length of the cell's record: 0 (unchanged), 3, 7, 14, 18, 23, 27, 37 or 41 */
TRT_ANSI_HD unsigned trt_delta256_half_record_bytes(const trt_delta_half_flags *f)
{
    if (!f->changed)
        return 0;
    return (trt_delta_half_starts(f) ? TRT_DELTA_CURSOR : 0) + trt_delta256_half_colour_bytes(f) + TRT_DELTA_HALF_GLYPH + (trt_delta_half_ends(f) ? TRT_DELTA_RESET : 0);
}

/* byte k < trt_delta256_half_record_bytes(f) of the record of cell (t, c) whose new indices are pair = upper | lower << 8.  Behind
 * the cursor (trt_delta_half_cursor_byte: a cell is one column wide) a record is a piece of the palette's half-block cell's 23 bytes
 * and of the row's end bytes behind them (trt_ansi256_half_cell_byte, 0..26): both colours are its bytes 0..19; the upper colour alone
 * its bytes 0..9 and the 'm' at 19; the lower colour alone its bytes 0, 1 and 11..19 ("\033[" in front of "48;5;"); the glyph its
 * bytes 20..22, the reset 23..26. */
TRT_ANSI_HD unsigned trt_delta256_half_record_byte(unsigned k, int t, int c, unsigned pair, const trt_delta_half_flags *f)
{
    const unsigned cursor = trt_delta_half_starts(f) ? TRT_DELTA_CURSOR : 0;
    if (k < cursor)
        return trt_delta_half_cursor_byte(k, t, c);
    k -= cursor;
    const unsigned colour = trt_delta256_half_colour_bytes(f);
    unsigned at;
    if (k >= colour)
        at = TRT_DELTA256_HALF_BOTH + (k - colour);
    else if (colour == TRT_DELTA256_HALF_BOTH)
        at = k;
    else if (trt_delta_half_upper(f))
        at = k < TRT_DELTA256_HALF_SINGLE - 1 ? k : TRT_DELTA256_HALF_BOTH - 1;
    else
        at = k < 2 ? k : k + (TRT_DELTA256_HALF_BOTH - TRT_DELTA256_HALF_SINGLE);
    return trt_ansi256_half_cell_byte((int)at, pair);
}

/* a lane's cells: their new indices (upper | lower << 8), what their records depend on, the records' lengths and their sum, and where
 * the cells lie */
typedef struct
{
    unsigned pair[TRT_DELTA_LANE_CELLS], bytes[TRT_DELTA_LANE_CELLS];
    trt_delta_half_flags flags[TRT_DELTA_LANE_CELLS];
    int trow[TRT_DELTA_LANE_CELLS], col[TRT_DELTA_LANE_CELLS];
    unsigned total;
} trt_delta256_half_lane;

/* The cells tile * TRT_DELTA_TILE + TRT_DELTA_LANE_CELLS * thread + j of a frame of width x rows pixels, (rows + 1) / 2 text rows; those
 * behind the frame have no record and are not loaded.  One 64-bit division per workgroup (where the tile starts), one 32-bit division
 * per lane.  Cell (t, col) has its upper pixel at pixel 2 t width + col of a frame and its lower one `width` pixels on, which exists,
 * and is loaded, when 2 t + 1 < rows; where it does not exist the index is TRT_XTERM256_BLACK in both frames.  The walk of
 * trt_delta_half_lane_cells, with the palette map between the loads and the compares. */
TRT_ANSI_HD trt_delta256_half_lane trt_delta256_half_lane_cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile,
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
    unsigned up[TRT_DELTA_LANE_CELLS + 2], low[TRT_DELTA_LANE_CELLS + 2], was_up[TRT_DELTA_LANE_CELLS + 2], was_low[TRT_DELTA_LANE_CELLS + 2];
    int there[TRT_DELTA_LANE_CELLS + 2], has_lower[TRT_DELTA_LANE_CELLS + 2], changed[TRT_DELTA_LANE_CELLS + 2];
    trt_delta256_half_lane c;
    /* all the loads, then the map: up to twenty-four pixels in flight at once, not a round trip per index */
    TRT_DELTA_UNROLL
    for (int j = -1; j <= TRT_DELTA_LANE_CELLS; j++)
    {
        there[j + 1] = col >= 0 && t < trows;
        has_lower[j + 1] = there[j + 1] && 2 * t + 1 < (unsigned long long)(unsigned)rows;
        const unsigned long long p = 2 * t * (unsigned)width + (unsigned)col; /* used only where `there` */
        up[j + 1] = there[j + 1] ? trt_delta_rgb(next, p) : 0u;
        low[j + 1] = has_lower[j + 1] ? trt_delta_rgb(next, p + (unsigned)width) : 0u;
        was_up[j + 1] = there[j + 1] ? trt_delta_rgb(shown, p) : 0u;
        was_low[j + 1] = has_lower[j + 1] ? trt_delta_rgb(shown, p + (unsigned)width) : 0u;
        if (j >= 0 && j < TRT_DELTA_LANE_CELLS)
        {
            c.trow[j] = (int)t;
            c.col[j] = col;
        }
        if (++col == width)
            col = 0, t++;
    }
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS + 2; j++)
    {
        up[j] = trt_xterm256_index_of(up[j]);
        was_up[j] = trt_xterm256_index_of(was_up[j]);
        low[j] = has_lower[j] ? trt_xterm256_index_of(low[j]) : (unsigned)TRT_XTERM256_BLACK;
        was_low[j] = has_lower[j] ? trt_xterm256_index_of(was_low[j]) : (unsigned)TRT_XTERM256_BLACK;
        changed[j] = there[j] && (up[j] != was_up[j] || low[j] != was_low[j]);
    }
    c.total = 0;
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.pair[j] = trt_ansi256_half_pair(up[j + 1], low[j + 1]);
        c.flags[j].changed = changed[j + 1];
        c.flags[j].changed_left = c.col[j] > 0 && changed[j];
        c.flags[j].changed_right = c.col[j] + 1 < width && changed[j + 2];
        c.flags[j].same_upper = up[j + 1] == up[j];
        c.flags[j].same_lower = low[j + 1] == low[j];
        c.bytes[j] = trt_delta256_half_record_bytes(&c.flags[j]);
        c.total += c.bytes[j];
    }
    return c;
}

/* byte k < c->bytes[j] of the record of the lane's j-th cell */
TRT_ANSI_HD unsigned trt_delta256_half_lane_byte(const trt_delta256_half_lane *c, int j, unsigned k)
{
    return trt_delta256_half_record_byte(k, c->trow[j], c->col[j], c->pair[j], &c->flags[j]);
}

#endif /* TRT_ANSI256_DELTA_HALF_H */
