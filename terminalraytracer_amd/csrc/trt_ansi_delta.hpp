// trt_ansi_delta.hpp -- the delta texts of a CHAIN of RGB8 frames (trt_ansi_delta_chain.h: a shown frame, n frames back to back, text b
// between frames b - 1 and b), written on the device: three launches in stream order whatever n is.  The text between two frames is a
// chain of one: there is no other set of kernels.  A text has one of two KINDS of cell: the full text's, two columns wide
// (trt_ansi_delta.h), and half-block cells, two pixel rows a cell (trt_ansi_delta_half.h).  Each header holds its format, the record
// lengths and bytes, and the LANE'S WALK: which bytes of the two frames a lane loads for its cells.  This file holds the tile scheme,
// once for all kinds: the prefix sum that gives every record its place.  Each of the two shapes of cell also exists in the xterm 256-colour
// palette (trt_ansi256_delta.h, trt_ansi256_delta_half.h): the same frames of RGB8 bytes, which the walk maps to palette indices itself, a
// cell changed where an INDEX differs; to this file two more kinds, nothing else.
//
//   measure   a grid of tiles x n, the pair in blockIdx.y: a workgroup per tile of TRT_DELTA_TILE cells (row-major; over the TEXT rows
//             for half-block cells), a lane per TRT_DELTA_LANE_CELLS consecutive cells: the kind's walk reads the pair's two frames and
//             sums the lengths of the lane's records, the wave is reduced (__shfl_down), the waves' sums added through LDS: one 32-bit
//             sum per tile (at most 1024 x 57 = 58 368)
//   offsets   ONE workgroup scans all n * tiles sums exclusively into 64-bit offsets, TRT_DELTA_SCAN_BLOCK sums per turn with a running
//             total, and stores the n texts' lengths
//   write     the grid and the walk again, an exclusive scan over the wave (__shfl_up), one over the waves' totals through LDS, and
//             every lane stores its records at tile offset + wave offset + lane offset, a byte at a time
//
// No workgroup waits for another one -- the order is the stream's -- and there is no atomic: a text is a function of its two frames, and
// the texts stand back to back.  Every byte below the lengths' sum is stored once and none behind it.  The frames and the texts may have
// any alignment: everything is read and stored by bytes; the lower row of an odd frame's last half-block text row is NOT loaded -- behind
// the shown frame is somebody else's memory, behind a frame of the chain the next one.  LDS: the waves' sums, nothing else.
#pragma once

#include "trt_ansi256_delta.h"
#include "trt_ansi256_delta_half.h"
#include "trt_ansi_delta.h"
#include "trt_ansi_delta_chain.h"
#include "trt_ansi_delta_half.h"
#include "trt_common.hpp"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// a kind of cell, to the tile scheme: the header's lane, its walk and its bytes
struct DeltaFull
{
    using Lane = trt_delta_lane;
    static __device__ __forceinline__ Lane cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile, unsigned thread)
    {
        return trt_delta_lane_cells(shown, next, width, rows, tile, thread);
    }
    static __device__ __forceinline__ unsigned byte(const Lane &c, int j, unsigned k) { return trt_delta_lane_byte(&c, j, k); }
};

struct DeltaHalf
{
    using Lane = trt_delta_half_lane;
    static __device__ __forceinline__ Lane cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile, unsigned thread)
    {
        return trt_delta_half_lane_cells(shown, next, width, rows, tile, thread);
    }
    static __device__ __forceinline__ unsigned byte(const Lane &c, int j, unsigned k) { return trt_delta_half_lane_byte(&c, j, k); }
};

struct Delta256Full
{
    using Lane = trt_delta256_lane;
    static __device__ __forceinline__ Lane cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile, unsigned thread)
    {
        return trt_delta256_lane_cells(shown, next, width, rows, tile, thread);
    }
    static __device__ __forceinline__ unsigned byte(const Lane &c, int j, unsigned k) { return trt_delta256_lane_byte(&c, j, k); }
};

struct Delta256Half
{
    using Lane = trt_delta256_half_lane;
    static __device__ __forceinline__ Lane cells(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned long long tile, unsigned thread)
    {
        return trt_delta256_half_lane_cells(shown, next, width, rows, tile, thread);
    }
    static __device__ __forceinline__ unsigned byte(const Lane &c, int j, unsigned k) { return trt_delta256_half_lane_byte(&c, j, k); }
};

template <class Kind>
__device__ __forceinline__ void delta_measure(const unsigned char *shown, const unsigned char *next, int width, int rows, unsigned *tile_bytes)
{
    __shared__ unsigned wave_bytes[TRT_DELTA_BLOCK / 64];
    unsigned sum = Kind::cells(shown, next, width, rows, blockIdx.x, threadIdx.x).total;
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
template <class Kind>
__device__ __forceinline__ void delta_write(const unsigned char *shown, const unsigned char *next, int width, int rows, const unsigned long long *tile_at,
                                            unsigned char *out, unsigned long long capacity)
{
    __shared__ unsigned wave_bytes[TRT_DELTA_BLOCK / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const typename Kind::Lane c = Kind::cells(shown, next, width, rows, blockIdx.x, threadIdx.x);
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
                out[at + k] = (unsigned char)Kind::byte(c, j, k);
        at += c.bytes[j];
    }
}

// The exclusive scan of `count` sums into 64-bit offsets that start at `base`, by ONE workgroup of TRT_DELTA_SCAN_BLOCK threads:
// TRT_DELTA_SCAN_BLOCK sums per turn with a running total, which every thread returns: base + all sums
__device__ __forceinline__ unsigned long long delta_scan(const unsigned *tile_bytes, unsigned long long count, unsigned long long base, unsigned long long *tile_at)
{
    __shared__ unsigned long long wave_bytes[TRT_DELTA_SCAN_BLOCK / 64];
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long running = base;
    for (unsigned long long first = 0; first < count; first += TRT_DELTA_SCAN_BLOCK)
    {
        const unsigned long long i = first + threadIdx.x, mine = i < count ? tile_bytes[i] : 0ull;
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
        if (i < count)
            tile_at[i] = running + before + through - mine;
        running += all;
        __syncthreads(); // the next turn overwrites the waves' sums
    }
    return running;
}

// ---- the kernels, on grids of dim3(tiles, n), blockIdx.y the pair (n = 1: the text between two frames): the bodies above, given the
// pair's two frames and the pair's slice of the tile arrays.  `out` and `capacity` are the whole buffer's: the offsets are the chain's ----

template <class Kind>
__device__ __forceinline__ void delta_chain_measure(const unsigned char *shown, const unsigned char *frames, int width, int rows, unsigned *tile_bytes)
{
    const trt_delta_chain_pair pair = trt_delta_chain_frames(shown, frames, width, rows, blockIdx.y);
    delta_measure<Kind>(pair.shown, pair.next, width, rows, tile_bytes + trt_delta_chain_tile(gridDim.x, blockIdx.y, 0));
}

template <class Kind>
__device__ __forceinline__ void delta_chain_write(const unsigned char *shown, const unsigned char *frames, int width, int rows, const unsigned long long *tile_at,
                                                  unsigned char *out, unsigned long long capacity)
{
    const trt_delta_chain_pair pair = trt_delta_chain_frames(shown, frames, width, rows, blockIdx.y);
    delta_write<Kind>(pair.shown, pair.next, width, rows, tile_at + trt_delta_chain_tile(gridDim.x, blockIdx.y, 0), out, capacity);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_chain_measure_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                  unsigned *tile_bytes)
{
    delta_chain_measure<DeltaFull>(shown, frames, width, rows, tile_bytes);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_half_chain_measure_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                       unsigned *tile_bytes)
{
    delta_chain_measure<DeltaHalf>(shown, frames, width, rows, tile_bytes);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_chain_write_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                const unsigned long long *tile_at, unsigned char *out, unsigned long long capacity)
{
    delta_chain_write<DeltaFull>(shown, frames, width, rows, tile_at, out, capacity);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi_delta_half_chain_write_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                     const unsigned long long *tile_at, unsigned char *out, unsigned long long capacity)
{
    delta_chain_write<DeltaHalf>(shown, frames, width, rows, tile_at, out, capacity);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi256_delta_chain_measure_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                     unsigned *tile_bytes)
{
    delta_chain_measure<Delta256Full>(shown, frames, width, rows, tile_bytes);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi256_delta_half_chain_measure_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                          unsigned *tile_bytes)
{
    delta_chain_measure<Delta256Half>(shown, frames, width, rows, tile_bytes);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi256_delta_chain_write_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                   const unsigned long long *tile_at, unsigned char *out, unsigned long long capacity)
{
    delta_chain_write<Delta256Full>(shown, frames, width, rows, tile_at, out, capacity);
}

__global__ __launch_bounds__(TRT_DELTA_BLOCK) void ansi256_delta_half_chain_write_kernel(const unsigned char *shown, const unsigned char *frames, int width, int rows,
                                                                                        const unsigned long long *tile_at, unsigned char *out, unsigned long long capacity)
{
    delta_chain_write<Delta256Half>(shown, frames, width, rows, tile_at, out, capacity);
}

// ONE workgroup of TRT_DELTA_SCAN_BLOCK threads: the scan over all n * tiles sums from `base`, a frame's first tile anywhere in a turn,
// then the n lengths, read from the offsets the workgroup itself has just stored
__global__ __launch_bounds__(TRT_DELTA_SCAN_BLOCK) void ansi_delta_chain_offsets_kernel(const unsigned *tile_bytes, unsigned long long tiles, unsigned n, unsigned long long base,
                                                                                       unsigned long long *tile_at, unsigned long long *text_bytes)
{
    const unsigned long long total = delta_scan(tile_bytes, n * tiles, base, tile_at);
    if (threadIdx.x < n) // the barrier that closes the scan's last turn stands between the other threads' stores and these loads
        text_bytes[threadIdx.x] = trt_delta_chain_text_bytes(tile_at, tiles, n, threadIdx.x, total);
}

// the length of a keyframe's text, which the host knows, to where the delta's length goes
__global__ void ansi_delta_keyframe_bytes_kernel(unsigned long long *text_bytes, unsigned long long bytes)
{
    *text_bytes = bytes;
}

#endif // TRT_UNIT_RENDER

} // namespace trt
