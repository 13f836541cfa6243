// trt_ansi256.hpp -- the frame as the terminal's text in the xterm 256-colour palette, written on the device: for the full text (two
// spaces a pixel) and the half-block text (two pixel rows a line) the kernels that stand in the ordered mean's place, the same
// formatting fed from RGB8 bytes, and the palette map alone, a byte a pixel.  trt_xterm256.h holds the palette map, trt_text_map.h the
// position map and the lane map, trt_ansi256.h and trt_ansi256_half.h the formats, trt_ansi.hpp the wave that carries them out
// (text_write); this file says what a lane of that wave holds of a cell and how a word fetches it.
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

// The ordered mean, the emitter's cast, the palette map and the 256-colour text in ONE pass, as the last kernel of a launch in
// reduce_samples_kernel's place: blockIdx.y is the frame, and it leaves the queue ready in the same way.  Frame b's text starts at
// out + b * trt_ansi256_text_bytes, aligned to nothing in general: every frame has a head and a tail of its own.  A single frame's grid
// has trt_text_waves(words of the text at `out`) waves; that of several frames the most waves an alignment needs (a frame's spare wave
// finds nothing to do).
__global__ __launch_bounds__(256) void reduce_samples_ansi256_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic, int spp,
                                                                     double inv_spp, unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long values = (long)width * rows * 3;
    const double *mine = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values;
    text_write<ansi256_text>(out + (size_t)blockIdx.y * (size_t)trt_ansi256_text_bytes(width, rows), width, rows, row_magic, 0u, t >> 6, (int)(t & 63),
                             [=](long long p) { return ansi_pixel_of_samples(mine, values, spp, inv_spp, p); });
}

// the same for the half-block text: frame b's starts at out + b * trt_ansi256_half_text_bytes
__global__ __launch_bounds__(256) void reduce_samples_ansi256_half_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                          unsigned width_magic, int spp, double inv_spp, unsigned int *queue, unsigned grid,
                                                                          unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long values = (long)width * rows * 3;
    const double *mine = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values;
    text_write<ansi256_half_text>(out + (size_t)blockIdx.y * (size_t)trt_ansi256_half_text_bytes(width, rows), width, rows, row_magic, width_magic, t >> 6,
                                  (int)(t & 63), [=](long long p, long long q) { return ansi_half_pixels_of_samples(mine, values, spp, inv_spp, p, q); });
}

// The formatting alone, of a frame that exists as RGB8 bytes rgb[p * 3 + channel] (trt_ansi256_from_rgb8_device; the reference-order
// kernel's frames, which have no scratch)
__global__ __launch_bounds__(256) void ansi256_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    text_write<ansi256_text>(out, width, rows, row_magic, 0u, t >> 6, (int)(t & 63), [=](long long p) {
        const unsigned char *px = rgb + 3 * p;
        return (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
    });
}

// the same for the half-block text (trt_ansi256_half_from_rgb8_device)
__global__ __launch_bounds__(256) void ansi256_half_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                     unsigned width_magic)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    text_write<ansi256_half_text>(out, width, rows, row_magic, width_magic, t >> 6, (int)(t & 63), [=](long long p, long long q) {
        const unsigned char *a = rgb + 3 * p, *b = rgb + 3 * q;
        ansi_half_pair both;
        both.upper = (unsigned)a[0] | (unsigned)a[1] << 8 | (unsigned)a[2] << 16;
        both.lower = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16;
        return both;
    });
}

// The palette map alone (trt_xterm256_from_rgb8_device): index[p] of the pixel rgb[3 p ...], a lane a pixel, any alignment of either
__global__ __launch_bounds__(256) void xterm256_from_rgb8_kernel(const unsigned char *rgb, unsigned char *index, unsigned long long pixels)
{
    const unsigned long long p = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < pixels)
        index[p] = (unsigned char)trt_xterm256_index(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
}

#endif // TRT_UNIT_RENDER

} // namespace trt
