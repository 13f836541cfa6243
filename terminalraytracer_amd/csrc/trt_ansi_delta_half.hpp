// trt_ansi_delta_half.hpp -- the delta text between two RGB8 frames in HALF-BLOCK cells, written on the device.  trt_ansi_delta_half.h
// holds the format, the record lengths and the record bytes; the scheme is that of trt_ansi_delta.hpp, whose offsets kernel and
// keyframe-length kernel serve this text as they are:
//
//   measure   a workgroup per tile of TRT_DELTA_TILE cells (row-major over the TEXT rows), a lane per TRT_DELTA_LANE_CELLS consecutive
//             cells: a cell's two pixels are read from owned rows 2 t and 2 t + 1 of both frames, the lengths of the lane's records
//             summed, the wave reduced (__shfl_down), the waves' sums added through LDS: one 32-bit sum per tile (at most 58 368)
//   offsets   ansi_delta_offsets_kernel
//   write     the lengths again, an exclusive scan over the wave (__shfl_up), one over the waves' totals through LDS, and every lane
//             stores its records at tile offset + wave offset + lane offset, a byte at a time
//
// No workgroup waits for another one and there is no atomic.  Every byte below the length is stored once and none behind it.  The
// frames and the text may have any alignment: everything is read and stored by bytes.  The lower row of an odd frame's last text row
// is NOT loaded -- behind the frame is somebody else's memory -- its pixels are black in both frames.  LDS: the waves' sums.
#pragma once

#include "trt_ansi_delta.hpp"
#include "trt_ansi_delta_half.h"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// a lane's cells: their new colours, what their records depend on, the records' lengths
struct DeltaHalfCells
{
    unsigned upper[TRT_DELTA_LANE_CELLS], lower[TRT_DELTA_LANE_CELLS], bytes[TRT_DELTA_LANE_CELLS];
    trt_delta_half_flags flags[TRT_DELTA_LANE_CELLS];
    int trow[TRT_DELTA_LANE_CELLS], col[TRT_DELTA_LANE_CELLS];
    unsigned total;
};

// The cells tile * TRT_DELTA_TILE + TRT_DELTA_LANE_CELLS * thread + j of a frame of `trows` text rows; those behind the frame have no
// record.  One 64-bit division per workgroup (where the tile starts), one 32-bit division per lane.  Cell (t, col) has its upper pixel
// at pixel 2 t width + col of a frame and its lower one `width` pixels on, which exists when 2 t + 1 < rows.
__device__ __forceinline__ DeltaHalfCells delta_half_cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile,
                                                           unsigned thread)
{
    const unsigned trows = ((unsigned)rows + 1u) / 2u;
    const unsigned long long tile_first = tile * TRT_DELTA_TILE;
    const unsigned long long tile_row = tile_first / (unsigned)width;
    const unsigned x = (unsigned)(tile_first - tile_row * (unsigned)width) + TRT_DELTA_LANE_CELLS * thread; // < 99 999 + 1024
    const unsigned q = x / (unsigned)width;
    // the lane's cells and a neighbour either side, [j + 1] the j-th: cell -1 only matters inside a row, so it is read only there
    unsigned long long t = tile_row + q;
    int col = (int)(x - q * (unsigned)width) - 1;
    unsigned up[TRT_DELTA_LANE_CELLS + 2], low[TRT_DELTA_LANE_CELLS + 2];
    bool changed[TRT_DELTA_LANE_CELLS + 2];
    DeltaHalfCells c;
#pragma unroll
    for (int j = -1; j <= TRT_DELTA_LANE_CELLS; j++)
    {
        const bool there = col >= 0 && t < trows;
        const bool has_lower = there && 2 * t + 1 < (unsigned long long)(unsigned)rows;
        const unsigned long long p = 2 * t * (unsigned)width + (unsigned)col; // used only where `there`
        up[j + 1] = there ? delta_rgb(next, p) : 0u;
        low[j + 1] = has_lower ? delta_rgb(next, p + (unsigned)width) : 0u;
        changed[j + 1] = there && (up[j + 1] != delta_rgb(shown, p) || (has_lower && low[j + 1] != delta_rgb(shown, p + (unsigned)width)));
        if (j >= 0 && j < TRT_DELTA_LANE_CELLS)
        {
            c.trow[j] = (int)t;
            c.col[j] = col;
        }
        if (++col == width)
            col = 0, t++;
    }
    c.total = 0;
#pragma unroll
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

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_half_measure_kernel(const unsigned char *shown, const unsigned char *next, int width, int rows,
                                                                                 unsigned *tile_bytes)
{
    __shared__ unsigned wave_bytes[TRT_DELTA_BLOCK / 64];
    unsigned sum = delta_half_cells(shown, next, width, rows, blockIdx.x, threadIdx.x).total;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        sum += (unsigned)__shfl_down((int)sum, d);
    if ((threadIdx.x & 63) == 0)
        wave_bytes[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        unsigned all = 0;
#pragma unroll
        for (int w = 0; w < TRT_DELTA_BLOCK / 64; w++)
            all += wave_bytes[w];
        tile_bytes[blockIdx.x] = all;
    }
}

// `capacity`: the bytes at `out`; a record that would end behind them is not stored (it cannot, if the capacity is the bound's)
__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_half_write_kernel(const unsigned char *shown, const unsigned char *next, int width, int rows,
                                                                               const unsigned long long *tile_at, unsigned char *out, unsigned long long capacity)
{
    __shared__ unsigned wave_bytes[TRT_DELTA_BLOCK / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DeltaHalfCells c = delta_half_cells(shown, next, width, rows, blockIdx.x, threadIdx.x);
    unsigned through = c.total; // inclusive over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const unsigned below = (unsigned)__shfl_up((int)through, d);
        if (lane >= (unsigned)d)
            through += below;
    }
    if (lane == 63)
        wave_bytes[wave] = through;
    __syncthreads();
    unsigned before = 0;
#pragma unroll
    for (unsigned w = 0; w < TRT_DELTA_BLOCK / 64; w++)
        before += w < wave ? wave_bytes[w] : 0u;
    unsigned long long at = tile_at[blockIdx.x] + before + (through - c.total);
#pragma unroll
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        if (at + c.bytes[j] <= capacity)
            for (unsigned k = 0; k < c.bytes[j]; k++)
                out[at + k] = (unsigned char)trt_delta_half_record_byte(k, c.trow[j], c.col[j], c.upper[j], c.lower[j], &c.flags[j]);
        at += c.bytes[j];
    }
}

#endif // TRT_UNIT_RENDER

} // namespace trt
