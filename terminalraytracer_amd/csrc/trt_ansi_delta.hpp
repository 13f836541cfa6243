// trt_ansi_delta.hpp -- the delta text between two RGB8 frames, written on the device: three launches in stream order.  trt_ansi_delta.h
// holds the format, the record lengths and the record bytes; this file the prefix sum that gives every record its place.
//
//   measure   a workgroup per tile of TRT_DELTA_TILE cells (row-major), a lane per TRT_DELTA_LANE_CELLS consecutive cells: both frames are
//             read, the lengths of the lane's records summed, the wave reduced (__shfl_down), the waves' sums added through LDS: one 32-bit
//             sum per tile (a tile's text is below 40 KB)
//   offsets   ONE workgroup scans the tiles' sums exclusively into 64-bit offsets, TRT_DELTA_SCAN_BLOCK sums per turn with a running
//             total, and stores the text's length
//   write     the lengths again, an exclusive scan over the wave (__shfl_up), one over the waves' totals through LDS, and every lane
//             stores its records at tile offset + wave offset + lane offset, a byte at a time
//
// No workgroup waits for another one -- the order is the stream's -- and there is no atomic: the text is a function of the two frames.
// Every byte below the length is stored once and none behind it.  The frames and the text may have any alignment: everything is
// read and stored by bytes.  LDS: the waves' sums, nothing else.
#pragma once

#include "trt_ansi_delta.h"
#include "trt_common.hpp"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// a lane's cells: their new colours, what their records depend on, the records' lengths, and where the first of them lies
struct DeltaCells
{
    unsigned rgb[TRT_DELTA_LANE_CELLS], bytes[TRT_DELTA_LANE_CELLS];
    trt_delta_flags flags[TRT_DELTA_LANE_CELLS];
    int row[TRT_DELTA_LANE_CELLS], col[TRT_DELTA_LANE_CELLS];
    unsigned total;
};

__device__ __forceinline__ unsigned delta_rgb(const unsigned char *frame, unsigned long long p)
{
    const unsigned char *px = frame + 3 * p;
    return (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
}

// The cells tile * TRT_DELTA_TILE + TRT_DELTA_LANE_CELLS * thread + j of a frame of `cells` cells; those behind the frame have no record.
// One 64-bit division per workgroup (where the tile starts), one 32-bit division per lane.
__device__ __forceinline__ DeltaCells delta_cells(const unsigned char *shown, const unsigned char *next, int width, unsigned long long cells, unsigned long long tile,
                                                  unsigned thread)
{
    const unsigned long long tile_first = tile * TRT_DELTA_TILE;
    const unsigned long long tile_row = tile_first / (unsigned)width;
    const unsigned x = (unsigned)(tile_first - tile_row * (unsigned)width) + TRT_DELTA_LANE_CELLS * thread; // < 49 999 + 1024
    const unsigned q = x / (unsigned)width;
    const unsigned long long p0 = tile_first + TRT_DELTA_LANE_CELLS * thread;
    int row = (int)(tile_row + q), col = (int)(x - q * (unsigned)width);
    // the lane's cells and a neighbour either side: [j + 1] is cell p0 + j
    unsigned now[TRT_DELTA_LANE_CELLS + 2];
    bool changed[TRT_DELTA_LANE_CELLS + 2];
#pragma unroll
    for (int j = -1; j <= TRT_DELTA_LANE_CELLS; j++)
    {
        const bool there = (j >= 0 || p0 > 0) && p0 + j < cells; // p0 + j wraps to a huge number only where p0 == 0, j == -1
        now[j + 1] = there ? delta_rgb(next, p0 + j) : 0u;
        changed[j + 1] = there && now[j + 1] != delta_rgb(shown, p0 + j);
    }
    DeltaCells c;
    c.total = 0;
#pragma unroll
    for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
    {
        c.rgb[j] = now[j + 1];
        c.row[j] = row;
        c.col[j] = col;
        c.flags[j].changed = changed[j + 1];
        c.flags[j].changed_left = col > 0 && changed[j];
        c.flags[j].changed_right = col + 1 < width && changed[j + 2];
        c.flags[j].same_as_left = now[j + 1] == now[j];
        c.bytes[j] = trt_delta_record_bytes(&c.flags[j]);
        c.total += c.bytes[j];
        if (++col == width)
            col = 0, row++;
    }
    return c;
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_measure_kernel(const unsigned char *shown, const unsigned char *next, int width, unsigned long long cells,
                                                                            unsigned *tile_bytes)
{
    __shared__ unsigned wave_bytes[TRT_DELTA_BLOCK / 64];
    unsigned sum = delta_cells(shown, next, width, cells, blockIdx.x, threadIdx.x).total;
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

// launched as ONE workgroup of TRT_DELTA_SCAN_BLOCK threads
__global__ __launch_bounds__(TRT_DELTA_SCAN_BLOCK) void ansi_delta_offsets_kernel(const unsigned *tile_bytes, unsigned long long tiles, unsigned long long *tile_at,
                                                                                 unsigned long long *text_bytes)
{
    __shared__ unsigned long long wave_bytes[TRT_DELTA_SCAN_BLOCK / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long running = 0;
    for (unsigned long long first = 0; first < tiles; first += TRT_DELTA_SCAN_BLOCK)
    {
        const unsigned long long i = first + threadIdx.x, mine = i < tiles ? tile_bytes[i] : 0ull;
        unsigned long long through = mine; // inclusive over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
        {
            const unsigned long long below = __shfl_up(through, d);
            if (lane >= (unsigned)d)
                through += below;
        }
        if (lane == 63)
            wave_bytes[wave] = through;
        __syncthreads();
        unsigned long long before = 0, all = 0;
#pragma unroll
        for (unsigned w = 0; w < TRT_DELTA_SCAN_BLOCK / 64; w++)
        {
            before += w < wave ? wave_bytes[w] : 0ull;
            all += wave_bytes[w];
        }
        if (i < tiles)
            tile_at[i] = running + before + through - mine;
        running += all;
        __syncthreads(); // the next turn overwrites the waves' sums
    }
    if (threadIdx.x == 0)
        *text_bytes = running;
}

// `capacity`: the bytes at `out`; a record that would end behind them is not stored (it cannot, if the capacity is the bound's)
__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_write_kernel(const unsigned char *shown, const unsigned char *next, int width, unsigned long long cells,
                                                                          const unsigned long long *tile_at, unsigned char *out, unsigned long long capacity)
{
    __shared__ unsigned wave_bytes[TRT_DELTA_BLOCK / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const DeltaCells c = delta_cells(shown, next, width, cells, blockIdx.x, threadIdx.x);
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
                out[at + k] = (unsigned char)trt_delta_record_byte(k, c.row[j], c.col[j], c.rgb[j], &c.flags[j]);
        at += c.bytes[j];
    }
}

// the length of a keyframe's text, which the host knows, to where the delta's length goes
__global__ void ansi_delta_keyframe_bytes_kernel(unsigned long long *text_bytes, unsigned long long bytes)
{
    *text_bytes = bytes;
}

#endif // TRT_UNIT_RENDER

} // namespace trt
