/*
 * trt_ansi256_delta.h -- the DELTA text of a frame in the xterm 256-COLOUR PALETTE: what a terminal that shows frame `shown` as the
 * text of trt_ansi256.h must be sent to show frame `next` (host + device, plain C).  The reference has no such emitter; this header is
 * the format's one specification in code, and trt_emitter_delta256_rgb8 (csrc/host/trt_emit.c) its sequential statement.
 *
 * Two frames of RGB8 bytes, rows x width x 3.  A pixel's INDEX is trt_xterm256_index_of of its three bytes (trt_xterm256.h).  Cell
 * (r, c) is CHANGED when its INDEX differs between the frames -- not when a byte does: a cell whose bytes move inside one palette
 * entry looks the same on the terminal and has no record.  A RUN is a maximal sequence of consecutive changed cells of one row.  The
 * text is the concatenation, rows ascending, cells left to right, of the RECORDS of the changed cells; an unchanged cell has none.  A
 * record is, in this order,
 *
 *   1. if the cell starts a run:  "\033[RRRRR;CCCCCH"          14 bytes, RRRRR = r + 1, CCCCC = 2 c + 1 (a cell is two columns wide)
 *   2. if it starts a run, or its new INDEX differs from the new index of the cell to its left:
 *                                 "\033[48;5;NNNm"             11 bytes, bytes 0..10 of the palette cell (trt_ansi256_cell_byte)
 *   3. always:                    two spaces                   bytes 11, 12 of the palette cell
 *   4. if it ends a run:          "\033[0m"                    bytes 13..16: the first four of a row's end bytes
 *
 * so parts 2..4 are bytes [from, to) of trt_ansi256_cell_byte, from = 0 or 11, to = 13 or 17, and a record is 2, 6, 13, 17, 27 or 31
 * bytes long -- a function of the cell and its two neighbours.  No prefix, no newline, no NUL; frames of equal indices give no text.
 *
 * The bound -- NOT that of trt_ansi_delta.h with other constants.  A run of L cells costs at most 14 + 11 L + 2 L + 4 = 18 + 13 L
 * bytes.  A row's runs are separated by at least one unchanged cell, so k runs hold at most width - (k - 1) cells: at most
 * 18 k + 13 (width - k + 1) = 13 width + 13 + 5 k bytes.  In trt_ansi_delta.h a run's fixed cost (18) is below a cell's (21), the
 * coefficient of k is negative and one run is worst; here it is ABOVE a cell's (13), so MORE runs cost more: the row is longest with
 * the most runs there can be, k = (width + 1) / 2 (k runs need k cells and k - 1 gaps: 2 k - 1 <= width):
 *
 *      13 width + 13 + 5 ((width + 1) / 2)  bytes per row, in integers: 31 at width 1, 44 at width 2.
 *
 * Changed and unchanged cells in turn reach it, every changed cell a run of one; an even width has one cell to spare, which makes
 * one of the runs two cells long (with different new indices).  tests/ansi256_delta_check.c goes through every pattern of changed
 * cells and equal neighbours for widths 1..12 and finds this to the byte.  It exceeds the whole palette text 6 + (13 width + 5) rows
 * for every size; the capacity is written as the larger of the two all the same, as trt_ansi_delta_capacity is.
 *
 * The limits.  Five decimal digits for r + 1 and for 2 c + 1: rows <= 99999, width <= 49999.
 *
 * How the device writes it: the scheme of trt_ansi_delta.h -- tiles of TRT_DELTA_TILE cells, TRT_DELTA_LANE_CELLS consecutive cells
 * per lane, lengths per cell, sums per tile (at most 1024 x 31 bytes), an exclusive scan of the tiles' sums, a scan inside the tile.
 * The LANE'S WALK is here, trt_delta256_lane_cells: which bytes of the two frames lane `thread` of tile `tile` loads and maps to
 * indices -- the frames stay RGB8, no paletted copy of a frame exists --, its cells' rows and columns across the end of a row, its
 * records' lengths; trt_delta256_lane_byte gives the bytes.  The kernels of trt_ansi_delta.hpp and tests/ansi256_delta_check.c call
 * the two as they call those of trt_ansi_delta.h.
 */
#ifndef TRT_ANSI256_DELTA_H
#define TRT_ANSI256_DELTA_H

#include "trt_ansi256.h"
#include "trt_ansi_delta.h"

#define TRT_DELTA256_COLOUR 11 /* strlen("\033[48;5;000m") */
#define TRT_DELTA256_RECORD_MAX (TRT_DELTA_CURSOR + TRT_DELTA256_COLOUR + TRT_DELTA_SPACES + TRT_DELTA_RESET) /* 31 */
#define TRT_DELTA256_MAX_ROWS TRT_DELTA_MAX_ROWS
#define TRT_DELTA256_MAX_WIDTH TRT_DELTA_MAX_WIDTH

TRT_ANSI_HD int trt_delta256_size_ok(int width, long long rows)
{
    return width > 0 && rows > 0 && width <= TRT_DELTA256_MAX_WIDTH && rows <= TRT_DELTA256_MAX_ROWS;
}

/* the most bytes a row of `width` cells can have: (width + 1) / 2 runs */
TRT_ANSI_HD unsigned long long trt_delta256_row_bound(int width)
{
    return 13ull * (unsigned)width + 13ull + 5ull * (((unsigned)width + 1u) / 2u);
}

/* the most bytes a palette delta text of width x rows can have; 0 for a screen that has none */
TRT_ANSI_HD unsigned long long trt_delta256_bound(int width, long long rows)
{
    if (!trt_delta256_size_ok(width, rows))
        return 0;
    return (unsigned long long)rows * trt_delta256_row_bound(width);
}

/* room for any text a palette delta entry writes: a delta or the keyframe, the whole palette text */
TRT_ANSI_HD unsigned long long trt_delta256_capacity(int width, long long rows)
{
    if (!trt_delta256_size_ok(width, rows))
        return 0;
    const unsigned long long whole = trt_ansi256_text_bytes(width, rows), bound = trt_delta256_bound(width, rows);
    return whole > bound ? whole : bound;
}

/* The neighbourhood of a cell is trt_delta_flags, same_as_left comparing the NEW INDICES; starts, ends and colours are those of
 * trt_ansi_delta.h.  Length of the cell's record: 0 (unchanged), 2, 6, 13, 17, 27 or 31 */
TRT_ANSI_HD unsigned trt_delta256_record_bytes(const trt_delta_flags *f)
{
    if (!f->changed)
        return 0;
    return (trt_delta_starts(f) ? TRT_DELTA_CURSOR : 0) + (trt_delta_colours(f) ? TRT_DELTA256_COLOUR : 0) + TRT_DELTA_SPACES +
           (trt_delta_ends(f) ? TRT_DELTA_RESET : 0);
}

/* byte k < trt_delta256_record_bytes(f) of the record of cell (r, c) whose new palette index is `index`; the cursor is the full
 * text's (trt_delta_cursor_byte: a cell is two columns wide) */
TRT_ANSI_HD unsigned trt_delta256_record_byte(unsigned k, int r, int c, unsigned index, const trt_delta_flags *f)
{
    const unsigned cursor = trt_delta_starts(f) ? TRT_DELTA_CURSOR : 0;
    if (k < cursor)
        return trt_delta_cursor_byte(k, r, c);
    return trt_ansi256_cell_byte((int)(k - cursor + (trt_delta_colours(f) ? 0 : TRT_DELTA256_COLOUR)), index);
}

/* a lane's cells: their new indices, what their records depend on, the records' lengths and their sum, and where the cells lie */
typedef struct
{
    unsigned index[TRT_DELTA_LANE_CELLS], bytes[TRT_DELTA_LANE_CELLS];
    trt_delta_flags flags[TRT_DELTA_LANE_CELLS];
    int row[TRT_DELTA_LANE_CELLS], col[TRT_DELTA_LANE_CELLS];
    unsigned total;
} trt_delta256_lane;

/* The cells tile * TRT_DELTA_TILE + TRT_DELTA_LANE_CELLS * thread + j of a frame of width x rows cells; those behind the frame have no
 * record and are not loaded.  One 64-bit division per workgroup (where the tile starts), one 32-bit division per lane.  The walk of
 * trt_delta_lane_cells, with the palette map between the loads and the compares. */
TRT_ANSI_HD trt_delta256_lane trt_delta256_lane_cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile, unsigned thread)
{
    const unsigned long long cells = (unsigned long long)(unsigned)width * (unsigned)rows;
    const unsigned long long tile_first = tile * TRT_DELTA_TILE;
    const unsigned long long tile_row = tile_first / (unsigned)width;
    const unsigned x = (unsigned)(tile_first - tile_row * (unsigned)width) + TRT_DELTA_LANE_CELLS * thread; /* < 49 999 + 1024 */
    const unsigned q = x / (unsigned)width;
    const unsigned long long p0 = tile_first + TRT_DELTA_LANE_CELLS * thread;
    int row = (int)(tile_row + q), col = (int)(x - q * (unsigned)width);
    /* the lane's cells and a neighbour either side: [j + 1] is cell p0 + j */
    unsigned now[TRT_DELTA_LANE_CELLS + 2], was[TRT_DELTA_LANE_CELLS + 2];
    int there[TRT_DELTA_LANE_CELLS + 2];
    trt_delta256_lane c;
    /* where the cells lie, in front of the loads, as in trt_delta_lane_cells: the loads' latency then covers the two divisions */
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.row[j] = row;
        c.col[j] = col;
        if (++col == width)
            col = 0, row++;
    }
    /* all the loads, then the map: twelve pixels in flight at once, not a round trip per index */
    TRT_DELTA_UNROLL
    for (int j = -1; j <= TRT_DELTA_LANE_CELLS; j++)
    {
        there[j + 1] = (j >= 0 || p0 > 0) && p0 + j < cells; /* p0 + j wraps to a huge number only where p0 == 0, j == -1 */
        now[j + 1] = there[j + 1] ? trt_delta_rgb(next, p0 + j) : 0u;
        was[j + 1] = there[j + 1] ? trt_delta_rgb(shown, p0 + j) : 0u;
    }
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS + 2; j++)
    {
        now[j] = trt_xterm256_index_of(now[j]);
        was[j] = trt_xterm256_index_of(was[j]);
    }
    c.total = 0;
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.index[j] = now[j + 1];
        c.flags[j].changed = there[j + 1] && now[j + 1] != was[j + 1];
        c.flags[j].changed_left = c.col[j] > 0 && there[j] && now[j] != was[j];
        c.flags[j].changed_right = c.col[j] + 1 < width && there[j + 2] && now[j + 2] != was[j + 2];
        c.flags[j].same_as_left = now[j + 1] == now[j];
        c.bytes[j] = trt_delta256_record_bytes(&c.flags[j]);
        c.total += c.bytes[j];
    }
    return c;
}

/* byte k < c->bytes[j] of the record of the lane's j-th cell */
TRT_ANSI_HD unsigned trt_delta256_lane_byte(const trt_delta256_lane *c, int j, unsigned k)
{
    return trt_delta256_record_byte(k, c->row[j], c->col[j], c->index[j], &c->flags[j]);
}

#endif /* TRT_ANSI256_DELTA_H */
