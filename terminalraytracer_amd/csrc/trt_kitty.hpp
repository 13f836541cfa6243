// trt_kitty.hpp -- the frame as a kitty graphics-protocol image, written on the device: the kernel that stands in the ordered mean's place
// when a host asks for true pixels in a terminal that takes them, and the same formatting fed from RGB8 bytes.  trt_kitty.h holds the
// format, its position map and its lane map; this file is the wave that carries them out.
//
// A wave owns 64 aligned words of the text, 256 consecutive bytes, and the up to 65 pixels they show.  Lane l forms pixel p0 + l ONCE --
// the ordered mean of its samples from 0.0 in sample order and the emitter's cast (rgb8_byte), or three bytes read from memory -- and
// keeps its four base64 characters as ONE register; where the payload is not 4-aligned the wave's last word shows a 65th pixel, which
// lane 63 forms beside its own.  Then every lane assembles its word: it finds the position of its first byte from the wave's (a
// compare), fetches the characters of the one or two pixels it shows from the lanes that hold them (__shfl: ds_bpermute_b32, no LDS is
// allocated), byte-aligns the two registers, or selects header and terminator literals by position, and stores the word.  No RGB8 frame
// and no frame of doubles is written on the way.  The only 64-bit division is trt_kitty_locate's, by a constant, once per wave.
#pragma once

#include "trt_ansi.hpp"
#include "trt_kitty.h"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// One wave's share of a frame's image text at `out` (any alignment).  Every lane of the wave calls it (the cross-lane reads need all of
// them); lanes store only what is theirs.  `pixel_rgb(p)`: r | g << 8 | b << 16 of pixel p < width * rows.
template <class Fetch>
__device__ __forceinline__ void kitty_write(unsigned char *out, int width, int rows, unsigned long long wave, int lane, Fetch pixel_rgb)
{
    const trt_kitty_shape shape = trt_kitty_shape_of(width, rows);
    const trt_text_split split = trt_text_split_of((unsigned long long)out, trt_kitty_text_bytes(width, rows));
    if (wave == 0 && lane < (int)split.head) // the head lies in the home prefix
    {
        const trt_kitty_at at = trt_kitty_locate((unsigned long long)lane);
        out[lane] = (unsigned char)trt_kitty_byte(&at, &shape, width, rows, 0u);
    }
    trt_kitty_wave w;
    if (!trt_kitty_wave_of(&split, &shape, wave, &w)) // the whole wave: a frame of a batch whose alignment needs a wave less than the grid has
        return;
    const unsigned mine = lane < w.count ? trt_kitty_chars(pixel_rgb(w.p0 + lane)) : 0u;
    unsigned extra = 0u; // the 65th pixel: one lane sums a second time
    if (w.count == TRT_KITTY_SPAN_PIXELS && lane == 63)
        extra = trt_kitty_chars(pixel_rgb(w.p0 + 64));
    extra = (unsigned)__shfl((int)extra, 63);

    const unsigned long long k = trt_text_lane_word(trt_kitty_kind(), wave, lane, 0);
    const trt_kitty_at at = trt_kitty_advance(&w.from, 4u * (unsigned)lane);
    int first, last;
    const int whole = trt_kitty_word_pixels(&at, &shape, &first, &last);
    const int rel_first = first - w.p0, rel_last = last - w.p0; // 0 .. 64 where the word shows a pixel
    const unsigned held_first = (unsigned)__shfl((int)mine, rel_first & 63), held_last = (unsigned)__shfl((int)mine, rel_last & 63);
    const unsigned word = trt_kitty_word(&at, &shape, width, rows, whole, first, rel_first == 64 ? extra : held_first, rel_last == 64 ? extra : held_last);
    unsigned char *const to = out + split.head + 4 * k; // (out + head) is 4-aligned
    if (k < split.words)
        *reinterpret_cast<unsigned *>(to) = word;
    else if (k == split.words) // the tail's slot: its bytes one by one
        for (unsigned b = 0; b < split.tail; b++)
            to[b] = (unsigned char)(word >> (8 * b));
}

// the wave of a thread, as a value the compiler knows to be the same in all of its lanes: what kitty_write finds once per wave -- the division, the
// wave's first pixel and its count -- then lives in scalar registers (a block is whole waves)
__device__ __forceinline__ unsigned long long kitty_wave_index()
{
    return (unsigned long long)blockIdx.x * (blockDim.x >> 6) + (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}

// pixel p of a frame's scratch, as ansi_pixel_of_samples (trt_ansi.hpp) forms it -- each sum from 0.0 in sample order, then the emitter's cast --
// with the loads of TWO samples in flight per lane, not four: the wave then fits into the 32 registers that four plain render waves leave a
// SIMD (profiles/r14/a_ordered_mean.md)
__device__ __forceinline__ unsigned kitty_pixel_of_samples(const double *samples, long values, int spp, double inv_spp, int p)
{
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    const double *s = samples + 3 * (long)p;
#pragma unroll 2
    for (int k = 0; k < spp; k++, s += values)
    {
        m0 += s[0];
        m1 += s[1];
        m2 += s[2];
    }
    return rgb8_byte(m0, inv_spp) | rgb8_byte(m1, inv_spp) << 8 | rgb8_byte(m2, inv_spp) << 16;
}

// The ordered mean, the emitter's cast and the image text in ONE pass, as the last kernel of a launch in reduce_samples_kernel's place:
// blockIdx.y is the frame, and it leaves the queue ready in the same way.  Frame b's text starts at out + b * trt_kitty_text_bytes,
// aligned to nothing in general: every frame has a head and a tail of its own.  A single frame's grid has trt_kitty_waves(out, bytes)
// waves; that of several frames trt_kitty_waves_most(bytes) (a frame's spare wave finds nothing to do).  The argument list is every
// whole text's (TextMeanKernel, trt_ansi.hpp): the image has no use for the two magics.
__global__ __launch_bounds__(256) void reduce_samples_kitty_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned, unsigned, int spp,
                                                                   double inv_spp, unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const long values = (long)width * rows * 3;
    const double *mine = samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values;
    kitty_write(out + (size_t)blockIdx.y * (size_t)trt_kitty_text_bytes(width, rows), width, rows, kitty_wave_index(), (int)(threadIdx.x & 63),
                [=](int p) { return kitty_pixel_of_samples(mine, values, spp, inv_spp, p); });
}

// The formatting alone, of a frame that exists as RGB8 bytes rgb[p * 3 + channel] (trt_kitty_from_rgb8_device; the reference-order
// kernel's frames, which have no scratch; TextFromRgb8Kernel's argument list)
__global__ __launch_bounds__(256) void kitty_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned, unsigned)
{
    kitty_write(out, width, rows, kitty_wave_index(), (int)(threadIdx.x & 63), pixels_of_rgb8{rgb});
}

#endif // TRT_UNIT_RENDER

} // namespace trt
