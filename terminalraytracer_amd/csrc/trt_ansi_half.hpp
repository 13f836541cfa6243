// trt_ansi_half.hpp -- the frame as the terminal's HALF-BLOCK text, written on the device: the kernel that stands in the ordered mean's
// place when a host asks for two pixel rows per line of text, and the same formatting fed from RGB8 bytes.  trt_text_map.h holds the
// position map and the lane map, trt_ansi_half.h the format, trt_ansi.hpp the wave that carries them out (text_write); this file says
// what a lane of that wave holds of a half-block cell and how a word fetches it.
//
// A wave owns TRT_ANSI_HALF_WAVE_WORDS aligned words of the text and the up to 61 cells they show.  Lane l forms BOTH pixels of cell
// C0 + l -- each the ordered mean of its samples from 0.0 in sample order and the emitter's cast (rgb8_byte), or three bytes read from
// memory, the two pixels' loads in flight together; the lower pixel of an odd frame's last row is 0 and is never read -- and keeps them
// packed in TWO registers.  A word fetches the two colours of its first byte's cell from the ONE lane that holds them (every digit of
// a word belongs to its first byte's cell, trt_ansi_half.h).  The lane's cell comes from the wave's by a compare or a multiply-high.
#pragma once

#include "trt_ansi.hpp"
#include "trt_ansi_half.h"

namespace trt
{

#ifdef TRT_UNIT_RENDER

struct ansi_half_pair
{
    unsigned upper, lower; // r | g << 8 | b << 16 each
};

// The half-block text for text_write: `pixels_rgb(p, q)` forms the pixels p and q < width * rows TOGETHER (the loads of both in flight
// at once).
struct ansi_half_text
{
    static constexpr int turns = TRT_ANSI_HALF_WAVE_WORDS / 64;
    using held = ansi_half_pair;
    using seen = ansi_half_pair;
    static __device__ __forceinline__ trt_text_kind kind() { return trt_ansi_half_kind(); }
    static __device__ __forceinline__ long long text_rows(int rows) { return trt_ansi_half_text_rows(rows); }
    static __device__ __forceinline__ unsigned long long text_bytes(int width, int rows) { return trt_ansi_half_text_bytes(width, rows); }
    static __device__ __forceinline__ unsigned lone_value(long long position, unsigned long long bytes) { return trt_ansi_half_lone_value(position, bytes); }

    template <class Fetch>
    static __device__ __forceinline__ held hold(const trt_text_at &from, int lane, int width, int rows, unsigned width_magic, Fetch pixels_rgb)
    {
        long long trow;
        int col;
        trt_ansi_half_lane_cell(&from, lane, width, width_magic, &trow, &col);
        held mine = {0u, 0u};
        if (2 * trow < rows)
        {
            // behind an odd frame's last row stands nothing of this frame: such a lane forms its upper pixel twice and keeps 0 for the lower
            const bool has_lower = 2 * trow + 1 < rows;
            const long long p = 2 * trow * width + col;
            const ansi_half_pair both = pixels_rgb(p, has_lower ? p + width : p);
            mine.upper = both.upper;
            mine.lower = has_lower ? both.lower : 0u;
        }
        return mine;
    }
    static __device__ __forceinline__ seen colours(const trt_text_at &at, const trt_text_at &, const trt_text_at &from, held mine, int width)
    {
        const int holder = (int)(trt_text_cell(&at, width) - trt_text_cell(&from, width)) & 63;
        seen shown;
        shown.upper = (unsigned)__shfl((int)mine.upper, holder);
        shown.lower = (unsigned)__shfl((int)mine.lower, holder);
        return shown;
    }
    // behind the first byte's cell stand no digits within a word
    static __device__ __forceinline__ unsigned byte(const trt_text_at &at, int, seen shown, unsigned) { return trt_ansi_half_byte(&at, shown.upper, shown.lower); }
};

// pixels p and q of a frame's scratch (as ansi_pixel_of_samples, trt_ansi.hpp, forms one): each sum from 0.0 in sample order, the two side by side
__device__ __forceinline__ ansi_half_pair ansi_half_pixels_of_samples(const double *samples, long values, int spp, double inv_spp, long long p, long long q)
{
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
#pragma unroll 2 // two samples of BOTH pixels in flight per lane, the sums in sample order (profiles/r13/a_half.md: one pixel after the other and four samples of both were slower)
    for (int k = 0; k < spp; k++)
    {
        const double *s = samples + (long)k * values;
        a0 += s[3 * p], a1 += s[3 * p + 1], a2 += s[3 * p + 2];
        b0 += s[3 * q], b1 += s[3 * q + 1], b2 += s[3 * q + 2];
    }
    ansi_half_pair both;
    both.upper = rgb8_byte(a0, inv_spp) | rgb8_byte(a1, inv_spp) << 8 | rgb8_byte(a2, inv_spp) << 16;
    both.lower = rgb8_byte(b0, inv_spp) | rgb8_byte(b1, inv_spp) << 8 | rgb8_byte(b2, inv_spp) << 16;
    return both;
}

// The ordered mean, the emitter's cast and the half-block text in ONE pass, as the last kernel of a launch in reduce_samples_kernel's
// place: blockIdx.y is the frame, and it leaves the queue ready in the same way.  Frame b's text starts at
// out + b * trt_ansi_half_text_bytes, aligned to nothing in general: every frame has a head and a tail of its own.  A single frame's
// grid has trt_text_waves(words of the text at `out`) waves; that of several frames the most waves an alignment needs.
__global__ __launch_bounds__(256) void reduce_samples_ansi_half_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                       unsigned width_magic, int spp, double inv_spp, unsigned int *queue, unsigned grid,
                                                                       unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long values = (long)width * rows * 3;
    const double *mine = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values;
    text_write<ansi_half_text>(out + (size_t)blockIdx.y * (size_t)trt_ansi_half_text_bytes(width, rows), width, rows, row_magic, width_magic, t >> 6, (int)(t & 63),
                               [=](long long p, long long q) { return ansi_half_pixels_of_samples(mine, values, spp, inv_spp, p, q); });
}

// The formatting alone, of a frame that exists as RGB8 bytes rgb[p * 3 + channel] (trt_ansi_half_from_rgb8_device; the reference-order
// kernel's frames, which have no scratch)
__global__ __launch_bounds__(256) void ansi_half_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                  unsigned width_magic)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    text_write<ansi_half_text>(out, width, rows, row_magic, width_magic, t >> 6, (int)(t & 63), [=](long long p, long long q) {
        const unsigned char *a = rgb + 3 * p, *b = rgb + 3 * q;
        ansi_half_pair both;
        both.upper = (unsigned)a[0] | (unsigned)a[1] << 8 | (unsigned)a[2] << 16;
        both.lower = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16;
        return both;
    });
}

#endif // TRT_UNIT_RENDER

} // namespace trt
