// trt_sixel.hpp -- the frame as a DEC sixel image, written on the device from the frame's RGB8 bytes: three kernels in stream order, the
// delta text's scheme (trt_ansi_delta.hpp), because the text's length depends on the picture.  trt_sixel.h holds the format, its position
// map and its lane map; this file carries them out.
//
//   measure   a workgroup per BAND of six pixel rows, a thread per column and every TRT_SIXEL_BLOCK-th behind it: the closed form
//             (trt_xterm256.h) maps each pixel's bytes to its palette index, which is ORed into the band's 240-bit mask in LDS (an LDS
//             atomic, and only where the index differs from the thread's last one); the workgroup stores the 8 mask words and their
//             popcount, the band's colour rows
//   offsets   ONE workgroup scans the bands' counts exclusively into 64-bit colour-row offsets (delta_scan: TRT_SIXEL_SCAN_BLOCK bands per
//             turn with a running total), stores the text's length, and writes what does not depend on the picture's colours: the 4350
//             bytes in front of the first colour row and the 2 behind the last
//   write     a workgroup per band and tile of TRT_SIXEL_BLOCK slots.  A thread forms the 6 x 4 palette indices its slot shows ONCE and
//             keeps them in six registers -- the closed form makes mapping the pixels a second time cheaper than an index frame in
//             memory -- then walks the band's mask in ascending order.  The mask words are made scalar (readfirstlane), so the walk is
//             the wave's, not the lane's: scalar bit-find, no divergence.  Per colour the thread stores one aligned 32-bit word; the slots
//             on a row's edges also carry bytes of "#NNN" and of the terminator, chosen by position, and the partial slots of a text that
//             is not 4-aligned store their bytes one by one.
//
// No workgroup waits for another -- the order is the stream's -- and no atomic touches global memory: the text is a function of the frame.
// Every byte below the length is stored exactly once and none at or behind it; the text may sit at any alignment and need not be
// initialised.  LDS: the 8 mask words, and the scan's waves' sums.
#pragma once

#include "trt_ansi_delta.hpp"
#include "trt_sixel.h"

namespace trt
{

#ifdef TRT_UNIT_RENDER

static_assert(TRT_SIXEL_SCAN_BLOCK == TRT_DELTA_SCAN_BLOCK, "the offsets kernel scans with delta_scan");

__global__ __launch_bounds__(TRT_SIXEL_BLOCK) void sixel_measure_kernel(const unsigned char *rgb, int width, int rows, unsigned *masks, unsigned *counts)
{
    __shared__ unsigned mask[TRT_SIXEL_MASK_WORDS];
    const int band = (int)blockIdx.x, band_rows = trt_sixel_band_rows(rows, band);
    if (threadIdx.x < TRT_SIXEL_MASK_WORDS)
        mask[threadIdx.x] = 0u;
    __syncthreads();
    unsigned last = 0u; // no index
    for (int column = (int)threadIdx.x; column < width; column += TRT_SIXEL_BLOCK)
        for (int j = 0; j < band_rows; j++)
        {
            const unsigned char *px = rgb + 3 * ((long long)(TRT_SIXEL_BAND * band + j) * width + column);
            const unsigned n = trt_xterm256_index(px[0], px[1], px[2]);
            if (n != last)
                atomicOr(&mask[(n - TRT_XTERM256_FIRST) >> 5], 1u << ((n - TRT_XTERM256_FIRST) & 31u));
            last = n;
        }
    __syncthreads();
    if (threadIdx.x < TRT_SIXEL_MASK_WORDS)
        masks[(size_t)TRT_SIXEL_MASK_WORDS * band + threadIdx.x] = mask[threadIdx.x];
    if (threadIdx.x == 0)
    {
        unsigned colours = 0;
#pragma unroll
        for (int w = 0; w < TRT_SIXEL_MASK_WORDS; w++)
            colours += (unsigned)__popc(mask[w]);
        counts[band] = colours;
    }
}

__global__ __launch_bounds__(TRT_SIXEL_SCAN_BLOCK) void sixel_offsets_kernel(const unsigned *counts, int width, int rows, unsigned long long *band_at, unsigned char *out,
                                                                             unsigned long long *text_bytes)
{
    const unsigned long long colour_rows = delta_scan(counts, (unsigned long long)trt_sixel_bands(rows), 0ull, band_at);
    const unsigned long long bytes = trt_sixel_text_bytes(width, colour_rows);
    for (unsigned at = threadIdx.x; at < TRT_SIXEL_PROLOGUE; at += TRT_SIXEL_SCAN_BLOCK)
        out[at] = (unsigned char)trt_sixel_prologue_byte(at, width, rows);
    if (threadIdx.x < TRT_SIXEL_END)
        out[bytes - TRT_SIXEL_END + threadIdx.x] = (unsigned char)trt_sixel_end_byte(threadIdx.x);
    if (threadIdx.x == 0)
        *text_bytes = bytes;
}

// grid: (the tiles of a colour row's slots, the bands)
__global__ __launch_bounds__(TRT_SIXEL_BLOCK) void sixel_write_kernel(const unsigned char *rgb, int width, int rows, const unsigned *masks, const unsigned long long *band_at,
                                                                      unsigned char *out)
{
    const int band = (int)blockIdx.y, row_bytes = trt_sixel_row_bytes(width);
    const trt_text_split split = trt_sixel_row_split((unsigned long long)out, width);
    const unsigned slot = blockIdx.x * TRT_SIXEL_BLOCK + threadIdx.x;
    if (slot >= trt_sixel_slots(&split)) // no barrier below
        return;
    const int first = trt_sixel_slot_first(&split, slot);
    const bool whole = first >= 0 && first + 4 <= row_bytes;
    const trt_sixel_lane lane = trt_sixel_lane_of(rgb, width, rows, band, first);
    unsigned mask[TRT_SIXEL_MASK_WORDS], left = 0; // the band's, the same in every lane: scalar registers
#pragma unroll
    for (int w = 0; w < TRT_SIXEL_MASK_WORDS; w++)
    {
        mask[w] = (unsigned)__builtin_amdgcn_readfirstlane((int)masks[(size_t)TRT_SIXEL_MASK_WORDS * band + w]);
        left += (unsigned)__popc(mask[w]);
    }
    const bool dashed = band + 1 < (int)gridDim.y; // not the last band: its last colour row ends in "-"
    unsigned char *to = out + TRT_SIXEL_PROLOGUE + (unsigned long long)row_bytes * band_at[band] + first; // 4-aligned where the slot is whole
#pragma unroll
    for (int w = 0; w < TRT_SIXEL_MASK_WORDS; w++)
        for (unsigned m = mask[w]; m; m &= m - 1u, to += row_bytes)
        {
            const unsigned n = trt_sixel_mask_index(w, __builtin_ctz(m));
            left--;
            const unsigned word = trt_sixel_lane_word(&lane, first, n, width, dashed && left == 0u);
            if (whole)
                *reinterpret_cast<unsigned *>(to) = word;
            else
                for (int i = 0; i < 4; i++)
                    if (first + i >= 0 && first + i < row_bytes)
                        to[i] = (unsigned char)(word >> (8 * i));
        }
}

#endif // TRT_UNIT_RENDER

} // namespace trt
