// trt_ansi.hpp -- the frame as the terminal's text, written on the device: the kernels that stand in the ordered mean's place when a
// host asks for what buffered_draw_screen would fwrite (TRT.c:1142-1172), and the same formatting fed from RGB8 bytes.  trt_ansi.h
// holds the layout and the lane map; this file the wave that carries them out.
//
// A wave owns TRT_ANSI_WAVE_WORDS aligned words of the text and the up to 63 pixels they show.  Lane l forms pixel P0 + l -- the
// ordered mean of its samples from 0.0 in sample order and the emitter's cast (rgb8_byte), or three bytes read from memory -- and keeps
// it packed in ONE register.  Then, six times, every lane assembles one word: it finds the position of its word's first byte from the
// wave's (32-bit arithmetic, trt_ansi_advance), walks the four bytes, fetches the one or two pixels they belong to from the lanes that
// hold them (__shfl: ds_bpermute_b32, no LDS is allocated) and stores the word: 64 lanes, 256 consecutive aligned bytes.  No RGB8
// frame and no frame of doubles is written on the way.  The only 64-bit division is trt_ansi_locate's, once per wave.
#pragma once

#include "trt_ansi.h"
#include "trt_common.hpp"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// One wave's share of a frame's text at `out` (any alignment).  `pixel_rgb(p)`: r | g << 8 | b << 16 of pixel p < width * rows.
// Every lane of the wave calls it (the cross-lane reads need all of them); lanes store only what is theirs.
template <class Fetch>
__device__ __forceinline__ void ansi_write(unsigned char *out, int width, int rows, unsigned row_magic, unsigned long long wave, int lane, Fetch pixel_rgb)
{
    const trt_ansi_split split = trt_ansi_split_of((unsigned long long)out, trt_ansi_text_bytes(width, rows));
    if (wave == 0)
    {
        const long long lone = trt_ansi_lone_byte(&split, lane);
        if (lone >= 0)
            out[lone] = (unsigned char)trt_ansi_lone_value(lone);
    }
    const unsigned long long first = trt_ansi_lane_word(wave, 0, 0);
    if (first >= split.words) // the whole wave: a frame of a batch whose alignment needs a wave less than the grid has
        return;
    const trt_ansi_at from = trt_ansi_locate(split.head + 4 * first, width, rows);
    const long long pixels = (long long)width * rows, p0 = trt_ansi_pixel(&from, width);
    const unsigned mine = p0 + lane < pixels ? pixel_rgb(p0 + lane) : 0u;
    unsigned char *const words = out + split.head;
#pragma unroll
    for (int j = 0; j < TRT_ANSI_WAVE_WORDS / 64; j++)
    {
        const unsigned long long k = trt_ansi_lane_word(wave, lane, j);
        trt_ansi_at at = trt_ansi_advance(&from, 4u * (unsigned)(64 * j + lane), width, rows, row_magic);
        trt_ansi_at walk = at;
        for (int b = 1; b < 4; b++)
            (void)trt_ansi_step(&walk, width, rows);
        // a word shows at most two pixels (a cell is longer than a word): that of its first byte and that of its last
        const unsigned rgb_a = (unsigned)__shfl((int)mine, (int)(trt_ansi_pixel(&at, width) - p0) & 63);
        const unsigned rgb_b = (unsigned)__shfl((int)mine, (int)(trt_ansi_pixel(&walk, width) - p0) & 63);
        unsigned word = trt_ansi_byte(&at, rows, rgb_a), other = 0;
        for (int b = 1; b < 4; b++)
        {
            other |= (unsigned)trt_ansi_step(&at, width, rows);
            word |= trt_ansi_byte(&at, rows, other ? rgb_b : rgb_a) << (8 * b);
        }
        if (k < split.words)
            *reinterpret_cast<unsigned *>(words + 4 * k) = word; // (out + head) is 4-aligned
    }
}

// pixel p of a frame's scratch samples[(k * pixels + p) * 3 + channel]: TRT.c:1063-1065, then the emitter's cast
__device__ __forceinline__ unsigned ansi_pixel_of_samples(const double *samples, long values, int spp, double inv_spp, long long p)
{
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
#pragma unroll 4 // the loads of four samples in flight per lane; the sums stay in sample order
    for (int k = 0; k < spp; k++)
    {
        const double *s = samples + ((long)k * values + 3 * p);
        m0 += s[0];
        m1 += s[1];
        m2 += s[2];
    }
    return rgb8_byte(m0, inv_spp) | rgb8_byte(m1, inv_spp) << 8 | rgb8_byte(m2, inv_spp) << 16;
}

// The ordered mean, the emitter's cast and the terminal's text in ONE pass, as the last kernel of a launch in reduce_samples_kernel's
// place: blockIdx.y is the frame, and it leaves the queue ready in the same way.  Frame b's text starts at out + b * trt_ansi_text_bytes,
// aligned to nothing in general: every frame has a head and a tail of its own.  A single frame's grid has trt_ansi_waves(words of the
// text at `out`) waves; that of several frames the most waves an alignment needs (a frame's spare wave finds nothing to do).
__global__ __launch_bounds__(256) void reduce_samples_ansi_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic, int spp,
                                                                  double inv_spp, unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long values = (long)width * rows * 3;
    const double *mine = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values;
    ansi_write(out + (size_t)blockIdx.y * (size_t)trt_ansi_text_bytes(width, rows), width, rows, row_magic, t >> 6, (int)(t & 63),
               [=](long long p) { return ansi_pixel_of_samples(mine, values, spp, inv_spp, p); });
}

// The formatting alone, of a frame that exists as RGB8 bytes rgb[p * 3 + channel] (trt_ansi_from_rgb8_device; the reference-order
// kernel's frames, which have no scratch)
__global__ __launch_bounds__(256) void ansi_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    ansi_write(out, width, rows, row_magic, t >> 6, (int)(t & 63), [=](long long p) {
        const unsigned char *px = rgb + 3 * p;
        return (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
    });
}

#endif // TRT_UNIT_RENDER

} // namespace trt
