/*
 * trt_ansi_delta_chain.h -- a CHAIN of delta texts: a shown frame and n frames of RGB8 bytes, rows x width x 3 each, and the n texts
 * that take a terminal from each frame to the next one, back to back (host + device, plain C).  Text b takes the terminal from frame
 * b - 1 to frame b; for b = 0 that is the shown frame.  1 <= n <= TRT_DELTA_CHAIN_MAX.
 *
 * A text is that of trt_ansi_delta.h or of trt_ansi_delta_half.h, its records and its lane's walk unchanged: text b depends on frames
 * b - 1 and b alone, so the n texts are ONE prefix sum over the tiles of n pairs of frames.  This header states the three things that
 * sum needs:
 *
 *   the frames   `frames` holds the n frames back to back, frame stride rows * width * 3 bytes, no padding, any alignment; `shown` is
 *                somewhere else.  PAIR b reads (shown, frame 0) for b = 0 and (frame b - 1, frame b) behind it:
 *                trt_delta_chain_frames.  Behind the last pixel row of frame b lies frame b + 1: the odd-frame rule of half-block
 *                cells holds per frame, because the kind's walk is given the frame's own `rows` and never loads a row 2 t + 1 >= rows.
 *   the tiles    tile t of pair b is entry b * tiles + t of the tile arrays, tiles = trt_delta_tiles(cells of one frame):
 *                trt_delta_chain_tile.  A pair's slice of the arrays is what the tile scheme of ONE pair indexes by its tile number.
 *   the texts    tile_at[] is the exclusive scan of all n * tiles sums, started from `base` (0, or the length of a text that stands
 *                in front of the chain's, a keyframe).  Text b starts at tile_at[b * tiles] and is as long as the difference to the
 *                next text's start, the scan's total for the last: trt_delta_chain_text_at, trt_delta_chain_text_bytes.  A text of 0
 *                bytes starts where the next one does.
 *
 * The kernels of trt_ansi_delta.hpp call these for (blockIdx.y, blockIdx.x); tests/ansi_delta_chain_check.c calls them on the host
 * for every pair, tile and thread, under the address sanitizer, with the n frames in one allocation to the byte.
 */
#ifndef TRT_ANSI_DELTA_CHAIN_H
#define TRT_ANSI_DELTA_CHAIN_H

#include "trt_ansi_delta.h"

#define TRT_DELTA_CHAIN_MAX 8 /* = TRT_BATCH_MAX (trt_hip.h); trt_render.hip holds the two against each other */

typedef struct
{
    const unsigned char *shown, *next;
} trt_delta_chain_pair;

/* bytes from a frame of the chain to the next one */
TRT_ANSI_HD unsigned long long trt_delta_chain_stride(int width, int rows) { return 3ull * (unsigned)width * (unsigned)rows; }

/* the two frames pair b < n compares */
TRT_ANSI_HD trt_delta_chain_pair trt_delta_chain_frames(const unsigned char *shown, const unsigned char *frames, int width, int rows, unsigned b)
{
    const unsigned long long stride = trt_delta_chain_stride(width, rows);
    trt_delta_chain_pair p;
    p.shown = b == 0 ? shown : frames + (b - 1) * stride;
    p.next = frames + b * stride;
    return p;
}

/* where tile t < tiles of pair b stands in the tile arrays */
TRT_ANSI_HD unsigned long long trt_delta_chain_tile(unsigned long long tiles, unsigned b, unsigned long long t) { return b * tiles + t; }

/* where text b < n starts, given the scan of the tiles' sums */
TRT_ANSI_HD unsigned long long trt_delta_chain_text_at(const unsigned long long *tile_at, unsigned long long tiles, unsigned b)
{
    return tile_at[trt_delta_chain_tile(tiles, b, 0)];
}

/* the length of text b < n; `total`: where the scan ended, base + all sums */
TRT_ANSI_HD unsigned long long trt_delta_chain_text_bytes(const unsigned long long *tile_at, unsigned long long tiles, unsigned n, unsigned b, unsigned long long total)
{
    return (b + 1 < n ? trt_delta_chain_text_at(tile_at, tiles, b + 1) : total) - trt_delta_chain_text_at(tile_at, tiles, b);
}

#endif /* TRT_ANSI_DELTA_CHAIN_H */
