// trt_ansi256.hpp -- the frame as the terminal's text in the xterm 256-colour palette, written on the device: the full text (two
// spaces a pixel) and the half-block text (two pixel rows a line), and the palette map alone, a byte a pixel.  trt_xterm256.h holds the
// palette map, trt_text_map.h the position map and the lane map, trt_ansi256.h and trt_ansi256_half.h the formats, trt_ansi.hpp the
// wave that carries them out (text_write), the fetches and the two kernels (reduce_samples_text_kernel, text_from_rgb8_kernel); this
// file says what a lane of that wave holds of a cell and how a word fetches it.
//
// A wave owns wave_words aligned words of the text (192: three a lane; 320: five a lane) and the up to 60 or 57 cells they show.  Lane
// l forms what cell C0 + l shows -- its pixel or its two pixels as the 24-bit texts' lanes form theirs: the ordered mean of the samples
// from 0.0 in sample order and the emitter's cast (rgb8_byte), or three bytes read from memory -- maps it to the palette ONCE and keeps
// the index or the two indices in ONE register.  A word fetches them from the one lane that holds its first byte's cell (every digit of
// a word belongs to that cell, trt_ansi256.h): one __shfl of 8 or 16 meaningful bits a word (ds_bpermute_b32, no LDS is allocated).
// No RGB8 frame and no frame of doubles is written on the way.
#pragma once

#include "trt_ansi.hpp"
#include "trt_ansi256.h"
#include "trt_ansi256_half.h"
#include "trt_ansi_half.hpp"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// The full 256-colour text for text_write: a lane holds ONE pixel's palette index, `pixel_rgb(p)`: r | g << 8 | b << 16 of pixel
// p < width * rows.  A text row is an owned row, so cell C0 + l is pixel C0 + l.
struct ansi256_text
{
    static constexpr int turns = TRT_ANSI256_WAVE_WORDS / 64;
    using held = unsigned;
    using seen = unsigned;
    static __device__ __forceinline__ trt_text_kind kind() { return trt_ansi256_kind(); }
    static __device__ __forceinline__ long long text_rows(int rows) { return trt_ansi256_text_rows(rows); }
    static __device__ __forceinline__ unsigned long long text_bytes(int width, int rows) { return trt_ansi256_text_bytes(width, rows); }
    static __device__ __forceinline__ unsigned lone_value(long long position, unsigned long long bytes) { return trt_ansi256_lone_value(position, bytes); }

    template <class Fetch>
    static __device__ __forceinline__ held hold(const trt_text_at &from, int lane, int width, int rows, unsigned, Fetch pixel_rgb)
    {
        const long long pixels = (long long)width * rows, p0 = trt_text_cell(&from, width);
        return p0 + lane < pixels ? trt_xterm256_index_of(pixel_rgb(p0 + lane)) : (unsigned)TRT_XTERM256_BLACK;
    }
    static __device__ __forceinline__ seen colours(const trt_text_at &at, const trt_text_at &, const trt_text_at &from, held mine, int width)
    {
        return (unsigned)__shfl((int)mine, (int)(trt_text_cell(&at, width) - trt_text_cell(&from, width)) & 63);
    }
    // behind the first byte's cell stand no digits within a word
    static __device__ __forceinline__ unsigned byte(const trt_text_at &at, int, seen shown, unsigned) { return trt_ansi256_byte(&at, shown); }
};

// The half-block 256-colour text for text_write: `pixels_rgb(p, q)` forms the pixels p and q < width * rows TOGETHER, as
// ansi_half_text's does (trt_ansi_half.hpp); a lane holds their two indices, upper | lower << 8.
struct ansi256_half_text
{
    static constexpr int turns = TRT_ANSI256_HALF_WAVE_WORDS / 64;
    using held = unsigned;
    using seen = unsigned;
    static __device__ __forceinline__ trt_text_kind kind() { return trt_ansi256_half_kind(); }
    static __device__ __forceinline__ long long text_rows(int rows) { return trt_ansi256_half_text_rows(rows); }
    static __device__ __forceinline__ unsigned long long text_bytes(int width, int rows) { return trt_ansi256_half_text_bytes(width, rows); }
    static __device__ __forceinline__ unsigned lone_value(long long position, unsigned long long bytes) { return trt_ansi256_half_lone_value(position, bytes); }

    template <class Fetch>
    static __device__ __forceinline__ held hold(const trt_text_at &from, int lane, int width, int rows, unsigned width_magic, Fetch pixels_rgb)
    {
        long long trow;
        int col;
        trt_ansi256_half_lane_cell(&from, lane, width, width_magic, &trow, &col);
        held mine = trt_ansi256_half_pair(TRT_XTERM256_BLACK, TRT_XTERM256_BLACK);
        if (2 * trow < rows)
        {
            // behind an odd frame's last row stands nothing of this frame: such a lane forms its upper pixel twice and keeps black for the lower
            const bool has_lower = 2 * trow + 1 < rows;
            const long long p = 2 * trow * width + col;
            const ansi_half_pair both = pixels_rgb(p, has_lower ? p + width : p);
            mine = trt_ansi256_half_pair(trt_xterm256_index_of(both.upper), has_lower ? trt_xterm256_index_of(both.lower) : (unsigned)TRT_XTERM256_BLACK);
        }
        return mine;
    }
    static __device__ __forceinline__ seen colours(const trt_text_at &at, const trt_text_at &, const trt_text_at &from, held mine, int width)
    {
        return (unsigned)__shfl((int)mine, (int)(trt_text_cell(&at, width) - trt_text_cell(&from, width)) & 63);
    }
    static __device__ __forceinline__ unsigned byte(const trt_text_at &at, int, seen shown, unsigned) { return trt_ansi256_half_byte(&at, shown); }
};

// The palette map alone (trt_xterm256_from_rgb8_device): index[p] of the pixel rgb[3 p ...], a lane a pixel, any alignment of either
__global__ __launch_bounds__(256) void xterm256_from_rgb8_kernel(const unsigned char *rgb, unsigned char *index, unsigned long long pixels)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < pixels)
        index[p] = (unsigned char)trt_xterm256_index(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
}

#endif // TRT_UNIT_RENDER

} // namespace trt
