// trt_ansi_half.hpp -- the frame as the terminal's HALF-BLOCK text, written on the device: the kernel that stands in the ordered mean's
// place when a host asks for two pixel rows per line of text, and the same formatting fed from RGB8 bytes.  trt_ansi_half.h holds the
// format, the layout and the lane map; this file the wave that carries them out, in the manner of trt_ansi.hpp.
//
// A wave owns TRT_ANSI_HALF_WAVE_WORDS aligned words of the text and the up to 61 cells they show.  Lane l forms BOTH pixels of cell
// C0 + l -- each the ordered mean of its samples from 0.0 in sample order and the emitter's cast (rgb8_byte), or three bytes read from
// memory, the two pixels' loads in flight together; the lower pixel of an odd frame's last row is 0 and is never read -- and keeps them
// packed in TWO registers.  Then, nine times, every lane assembles one word: it finds the position of its word's first byte from the wave's (32-bit arithmetic,
// trt_ansi_half_advance), fetches the two colours of that byte's cell from the lane that holds them (__shfl: ds_bpermute_b32, no LDS
// is allocated; every digit of a word belongs to its first byte's cell, trt_ansi_half.h), walks the four bytes and stores the word: 64
// lanes, 256 consecutive aligned bytes.  No RGB8 frame and no frame of doubles is written on the way.  The only 64-bit division is
// trt_ansi_half_locate's, once per wave; the lane's cell comes from the wave's by a compare or a multiply-high.
#pragma once

#include "trt_ansi_half.h"
#include "trt_common.hpp"

namespace trt
{

#ifdef TRT_UNIT_RENDER

struct ansi_half_pair
{
    unsigned upper, lower; // r | g << 8 | b << 16 each
};

// One wave's share of a frame's text at `out` (any alignment).  `pixels_rgb(p, q)`: the pixels p and q < width * rows, formed TOGETHER
// (the loads of both in flight at once).  Every lane of the wave calls it (the cross-lane reads need all of them); lanes store only
// what is theirs.
template <class Fetch>
__device__ __forceinline__ void ansi_half_write(unsigned char *out, int width, int rows, unsigned row_magic, unsigned width_magic, unsigned long long wave, int lane,
                                                Fetch pixels_rgb)
{
    const unsigned long long bytes = trt_ansi_half_text_bytes(width, rows);
    const trt_ansi_half_split split = trt_ansi_half_split_of((unsigned long long)out, bytes);
    if (wave == 0)
    {
        const long long lone = trt_ansi_half_lone_byte(&split, lane);
        if (lone >= 0)
            out[lone] = (unsigned char)trt_ansi_half_lone_value(lone, bytes);
    }
    const unsigned long long first = trt_ansi_half_lane_word(wave, 0, 0);
    if (first >= split.words) // the whole wave: a frame of a batch whose alignment needs a wave less than the grid has
        return;
    const trt_ansi_half_at from = trt_ansi_half_locate(split.head + 4 * first, width, rows);
    const long long c0 = trt_ansi_half_cell(&from, width);
    long long trow;
    int col;
    trt_ansi_half_lane_cell(&from, lane, width, width_magic, &trow, &col);
    unsigned upper = 0u, lower = 0u;
    if (2 * trow < rows)
    {
        // behind an odd frame's last row stands nothing of this frame: such a lane forms its upper pixel twice and keeps 0 for the lower
        const bool has_lower = 2 * trow + 1 < rows;
        const long long p = 2 * trow * width + col;
        const ansi_half_pair both = pixels_rgb(p, has_lower ? p + width : p);
        upper = both.upper;
        lower = has_lower ? both.lower : 0u;
    }
    unsigned char *const words = out + split.head;
#pragma unroll
    for (int j = 0; j < TRT_ANSI_HALF_WAVE_WORDS / 64; j++)
    {
        const unsigned long long k = trt_ansi_half_lane_word(wave, lane, j);
        trt_ansi_half_at at = trt_ansi_half_advance(&from, 4u * (unsigned)(64 * j + lane), width, rows, row_magic);
        const int holder = (int)(trt_ansi_half_cell(&at, width) - c0) & 63;
        const unsigned up = (unsigned)__shfl((int)upper, holder), lo = (unsigned)__shfl((int)lower, holder);
        unsigned word = trt_ansi_half_byte(&at, up, lo);
        for (int b = 1; b < 4; b++)
        {
            (void)trt_ansi_half_step(&at, width, rows);
            word |= trt_ansi_half_byte(&at, up, lo) << (8 * b); // behind the first byte's cell stand no digits within a word
        }
        if (k < split.words)
            *reinterpret_cast<unsigned *>(words + 4 * k) = word; // (out + head) is 4-aligned
    }
}

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
// grid has trt_ansi_half_waves(words of the text at `out`) waves; that of several frames the most waves an alignment needs.
__global__ __launch_bounds__(256) void reduce_samples_ansi_half_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                       unsigned width_magic, int spp, double inv_spp, unsigned int *queue, unsigned grid,
                                                                       unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long values = (long)width * rows * 3;
    const double *mine = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values;
    ansi_half_write(out + (size_t)blockIdx.y * (size_t)trt_ansi_half_text_bytes(width, rows), width, rows, row_magic, width_magic, t >> 6, (int)(t & 63),
                    [=](long long p, long long q) { return ansi_half_pixels_of_samples(mine, values, spp, inv_spp, p, q); });
}

// The formatting alone, of a frame that exists as RGB8 bytes rgb[p * 3 + channel] (trt_ansi_half_from_rgb8_device; the reference-order
// kernel's frames, which have no scratch)
__global__ __launch_bounds__(256) void ansi_half_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                  unsigned width_magic)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    ansi_half_write(out, width, rows, row_magic, width_magic, t >> 6, (int)(t & 63), [=](long long p, long long q) {
        const unsigned char *a = rgb + 3 * p, *b = rgb + 3 * q;
        ansi_half_pair both;
        both.upper = (unsigned)a[0] | (unsigned)a[1] << 8 | (unsigned)a[2] << 16;
        both.lower = (unsigned)b[0] | (unsigned)b[1] << 8 | (unsigned)b[2] << 16;
        return both;
    });
}

#endif // TRT_UNIT_RENDER

} // namespace trt
