/*
 * trt_ansi_delta.h -- the DELTA text of a frame: what a terminal that shows frame `shown` must be sent to show frame `next`
 * (host + device, plain C).  The reference has no such emitter (buffered_draw_screen, TRT.c:1142-1172, repaints every cell of every
 * frame); this header is the format's one specification in code.
 *
 * Two frames of RGB8 bytes, rows x width x 3.  Cell (r, c) is CHANGED when its three bytes differ.  A RUN is a maximal sequence of
 * consecutive changed cells of one row.  The text is the concatenation, rows ascending, cells left to right, of the RECORDS of the
 * changed cells; an unchanged cell has none.  A record is, in this order,
 *
 *   1. if the cell starts a run:  "\033[RRRRR;CCCCCH"          14 bytes, RRRRR = r + 1, CCCCC = 2 c + 1 (a cell is two columns wide)
 *   2. if it starts a run, or its new colour differs from the new colour of the cell to its left:
 *                                 "\033[48;2;RRR;GGG;BBBm"     19 bytes, bytes 0..18 of the reference's pixel_str (trt_ansi_cell_byte)
 *   3. always:                    two spaces                   bytes 19, 20 of pixel_str
 *   4. if it ends a run:          "\033[0m"                    bytes 21..24 of pixel_str
 *
 * so parts 2..4 are bytes [from, to) of the cell's 25 bytes in the full text, from = 0 or 19, to = 21 or 25, and a record is 2, 6, 21,
 * 25, 35 or 39 bytes long -- a function of the cell and its two neighbours.  No prefix, no newline, no NUL; equal frames give no text.
 *
 * The bound.  A run of L cells costs at most 14 + 19 L + 2 L + 4 = 18 + 21 L bytes.  A row's runs are separated by at least one
 * unchanged cell, so k runs hold at most width - (k - 1) cells: at most 18 k + 21 (width - k + 1) = 21 width + 21 - 3 k bytes, largest
 * at k = 1: 21 width + 18 per row.  A frame whose every cell changed and whose horizontal neighbours all differ reaches it.
 *
 * The limits.  Five decimal digits for r + 1 and for 2 c + 1: rows <= 99999, width <= 49999.
 *
 * How the device writes it: cells are numbered row-major, a TILE is TRT_DELTA_TILE consecutive cells, a lane owns TRT_DELTA_LANE_CELLS
 * consecutive cells of it.  Lengths per cell, sums per tile, an exclusive scan of the tiles' sums, a scan inside the tile: a record's
 * place is a prefix sum over the frame.  The LANE'S WALK is here, trt_delta_lane_cells: which bytes of the two frames lane `thread` of
 * tile `tile` loads, its cells' rows and columns across the end of a row, its records' lengths; trt_delta_lane_byte gives the bytes.
 * The kernels of trt_ansi_delta.hpp call the two for (blockIdx.x, threadIdx.x) and add the tile scheme, the sums and scans over the
 * lanes; tests/ansi_delta_check.c calls the same two for every tile and every thread 0 .. TRT_DELTA_BLOCK - 1 on the host, under the
 * address sanitizer, with frames allocated to the byte.
 */
#ifndef TRT_ANSI_DELTA_H
#define TRT_ANSI_DELTA_H

#include "trt_ansi.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_DELTA_UNROLL _Pragma("unroll")
#else
#define TRT_DELTA_UNROLL /* the host compiler is left to itself */
#endif

#define TRT_DELTA_CURSOR 14 /* strlen("\033[00001;00001H") */
#define TRT_DELTA_COLOUR 19 /* strlen("\033[48;2;000;000;000m") */
#define TRT_DELTA_SPACES 2
#define TRT_DELTA_RESET 4 /* strlen("\033[0m") */
#define TRT_DELTA_RECORD_MAX (TRT_DELTA_CURSOR + TRT_DELTA_COLOUR + TRT_DELTA_SPACES + TRT_DELTA_RESET) /* 39 */
#define TRT_DELTA_MAX_ROWS 99999
#define TRT_DELTA_MAX_WIDTH 49999
#define TRT_DELTA_LANE_CELLS 4
#define TRT_DELTA_BLOCK 256                                          /* threads of a workgroup of the measure and write kernels */
#define TRT_DELTA_TILE (TRT_DELTA_BLOCK * TRT_DELTA_LANE_CELLS)      /* cells of a workgroup: at most 39 936 bytes of text */
#define TRT_DELTA_SCAN_BLOCK 1024                                    /* threads of the one workgroup that scans the tiles' sums */

/* the neighbourhood of a cell a record depends on.  changed_left is 0 in column 0, changed_right 0 in the last column; same_as_left
 * compares the NEW colours and means nothing in column 0 (a run starts there) */
typedef struct
{
    int changed_left, changed, changed_right, same_as_left;
} trt_delta_flags;

TRT_ANSI_HD int trt_delta_size_ok(int width, long long rows)
{
    return width > 0 && rows > 0 && width <= TRT_DELTA_MAX_WIDTH && rows <= TRT_DELTA_MAX_ROWS;
}

/* the most bytes a delta text of width x rows can have; 0 for a screen that has none */
TRT_ANSI_HD unsigned long long trt_delta_bound(int width, long long rows)
{
    if (!trt_delta_size_ok(width, rows))
        return 0;
    return (unsigned long long)rows * (21ull * (unsigned)width + 18ull);
}

TRT_ANSI_HD int trt_delta_starts(const trt_delta_flags *f) { return f->changed && !f->changed_left; }
TRT_ANSI_HD int trt_delta_ends(const trt_delta_flags *f) { return f->changed && !f->changed_right; }
TRT_ANSI_HD int trt_delta_colours(const trt_delta_flags *f) { return f->changed && (!f->changed_left || !f->same_as_left); }

/* length of the cell's record: 0 (unchanged), 2, 6, 21, 25, 35 or 39 */
TRT_ANSI_HD unsigned trt_delta_record_bytes(const trt_delta_flags *f)
{
    if (!f->changed)
        return 0;
    return (trt_delta_starts(f) ? TRT_DELTA_CURSOR : 0) + (trt_delta_colours(f) ? TRT_DELTA_COLOUR : 0) + TRT_DELTA_SPACES +
           (trt_delta_ends(f) ? TRT_DELTA_RESET : 0);
}

/* byte k < 14 of the cursor address of cell (r, c) */
TRT_ANSI_HD unsigned trt_delta_cursor_byte(unsigned k, int r, int c)
{
    const unsigned long long k0 = TRT_ANSI_PACK8(0x1b, '[', '0', '0', '0', '0', '0', ';'), k1 = TRT_ANSI_PACK8('0', '0', '0', '0', '0', 'H', 0, 0);
    const unsigned d = k < 8 ? k - 2 : k - 8; /* digits at 2..6 and 8..12, most significant first */
    const unsigned v = k < 8 ? (unsigned)r + 1u : 2u * (unsigned)c + 1u;
    const unsigned digit = d == 0 ? v / 10000u : d == 1 ? (v / 1000u) % 10u : d == 2 ? (v / 100u) % 10u : d == 3 ? (v / 10u) % 10u : v % 10u;
    return ((unsigned)((k < 8 ? k0 : k1) >> ((k & 7) * 8)) & 0xffu) + (d < 5u ? digit : 0u);
}

/* byte k < trt_delta_record_bytes(f) of the record of cell (r, c) whose new colour is rgb = r | g << 8 | b << 16 */
TRT_ANSI_HD unsigned trt_delta_record_byte(unsigned k, int r, int c, unsigned rgb, const trt_delta_flags *f)
{
    const unsigned cursor = trt_delta_starts(f) ? TRT_DELTA_CURSOR : 0;
    if (k < cursor)
        return trt_delta_cursor_byte(k, r, c);
    return trt_ansi_cell_byte((int)(k - cursor + (trt_delta_colours(f) ? 0 : TRT_DELTA_COLOUR)), rgb);
}

/* tiles of a frame of `cells` cells */
TRT_ANSI_HD unsigned long long trt_delta_tiles(unsigned long long cells) { return (cells + TRT_DELTA_TILE - 1) / TRT_DELTA_TILE; }

/* a lane's cells: their new colours, what their records depend on, the records' lengths and their sum, and where the cells lie */
typedef struct
{
    unsigned rgb[TRT_DELTA_LANE_CELLS], bytes[TRT_DELTA_LANE_CELLS];
    trt_delta_flags flags[TRT_DELTA_LANE_CELLS];
    int row[TRT_DELTA_LANE_CELLS], col[TRT_DELTA_LANE_CELLS];
    unsigned total;
} trt_delta_lane;

/* pixel p of a frame as r | g << 8 | b << 16, by bytes */
TRT_ANSI_HD unsigned trt_delta_rgb(const unsigned char *frame, unsigned long long p)
{
    const unsigned char *px = frame + 3 * p;
    return (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
}

/* The cells tile * TRT_DELTA_TILE + TRT_DELTA_LANE_CELLS * thread + j of a frame of width x rows cells; those behind the frame have no
 * record and are not loaded.  One 64-bit division per workgroup (where the tile starts), one 32-bit division per lane. */
TRT_ANSI_HD trt_delta_lane trt_delta_lane_cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile, unsigned thread)
{
    const unsigned long long cells = (unsigned long long)(unsigned)width * (unsigned)rows;
    const unsigned long long tile_first = tile * TRT_DELTA_TILE;
    const unsigned long long tile_row = tile_first / (unsigned)width;
    const unsigned x = (unsigned)(tile_first - tile_row * (unsigned)width) + TRT_DELTA_LANE_CELLS * thread; /* < 49 999 + 1024 */
    const unsigned q = x / (unsigned)width;
    const unsigned long long p0 = tile_first + TRT_DELTA_LANE_CELLS * thread;
    int row = (int)(tile_row + q), col = (int)(x - q * (unsigned)width);
    /* the lane's cells and a neighbour either side: [j + 1] is cell p0 + j */
    unsigned now[TRT_DELTA_LANE_CELLS + 2];
    int changed[TRT_DELTA_LANE_CELLS + 2];
    trt_delta_lane c;
    /* where the cells lie, in front of the loads: the device compiler then issues the two divisions before and among the loads, whose
     * latency covers them; with the rows and columns formed behind the loads it sinks the divisions behind the last wait */
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.row[j] = row;
        c.col[j] = col;
        if (++col == width)
            col = 0, row++;
    }
    TRT_DELTA_UNROLL
    for (int j = -1; j <= TRT_DELTA_LANE_CELLS; j++)
    {
        const int there = (j >= 0 || p0 > 0) && p0 + j < cells; /* p0 + j wraps to a huge number only where p0 == 0, j == -1 */
        now[j + 1] = there ? trt_delta_rgb(next, p0 + j) : 0u;
        changed[j + 1] = there && now[j + 1] != trt_delta_rgb(shown, p0 + j);
    }
    c.total = 0;
    TRT_DELTA_UNROLL
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.rgb[j] = now[j + 1];
        c.flags[j].changed = changed[j + 1];
        c.flags[j].changed_left = c.col[j] > 0 && changed[j];
        c.flags[j].changed_right = c.col[j] + 1 < width && changed[j + 2];
        c.flags[j].same_as_left = now[j + 1] == now[j];
        c.bytes[j] = trt_delta_record_bytes(&c.flags[j]);
        c.total += c.bytes[j];
    }
    return c;
}

/* byte k < c->bytes[j] of the record of the lane's j-th cell */
TRT_ANSI_HD unsigned trt_delta_lane_byte(const trt_delta_lane *c, int j, unsigned k)
{
    return trt_delta_record_byte(k, c->row[j], c->col[j], c->rgb[j], &c->flags[j]);
}

#endif /* TRT_ANSI_DELTA_H */
