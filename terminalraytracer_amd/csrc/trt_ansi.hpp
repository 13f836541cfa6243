// trt_ansi.hpp -- the frame as the terminal's text, written on the device: the wave that writes a whole text of either format
// (text_write), what it fetches a cell's pixels from (the scratch or RGB8 bytes), the two kernels every character-cell text is an
// instantiation of -- the one that stands in the ordered mean's place when a host asks for what buffered_draw_screen would fwrite
// (TRT.c:1142-1172), and the same formatting fed from RGB8 bytes -- and the full text's format.  trt_text_map.h holds the position map
// and the lane map, trt_ansi.h the format; trt_ansi_half.hpp and trt_ansi256.hpp say what the other formats' lanes hold.
//
// A wave owns wave_words aligned words of the text and the up to 63 cells they show.  Lane l forms what cell C0 + l shows -- the full
// text's one pixel, the ordered mean of its samples from 0.0 in sample order and the emitter's cast (rgb8_byte), or three bytes read
// from memory -- and keeps it packed in registers.  Then, wave_words / 64 times, every lane assembles one word: it finds the position
// of its word's first byte from the wave's (32-bit arithmetic, trt_text_advance), fetches the colours its four bytes show from the
// lanes that hold them (__shfl: ds_bpermute_b32, no LDS is allocated), walks the four bytes and stores the word: 64 lanes, 256
// consecutive aligned bytes.  No RGB8 frame and no frame of doubles is written on the way.  The only 64-bit division is
// trt_text_locate's, once per wave.
#pragma once

#include "trt_ansi.h"
#include "trt_common.hpp"

namespace trt
{

#ifdef TRT_UNIT_RENDER

// One wave's share of a frame's text at `out` (any alignment).  Every lane of the wave calls it (the cross-lane reads need all of
// them); lanes store only what is theirs.  The Format says what is its own:
//   kind(), text_rows, text_bytes, lone_value      the format header's
//   turns                                          kind().wave_words / 64, for the unrolling
//   hold(from, lane, ..., fetch) -> held           what the lane keeps of cell trt_text_cell(from) + lane, formed through `fetch`
//   colours(at, last, from, mine, width) -> seen   what the word from at to last shows, fetched from the lanes that hold it
//   byte(at, rows, seen, other)                    what stands at *at; `other`: the walk has left the cell of the word's first byte
template <class Format, class Fetch>
__device__ __forceinline__ void text_write(unsigned char *out, int width, int rows, unsigned row_magic, unsigned width_magic, unsigned long long wave, int lane,
                                           Fetch fetch)
{
    const trt_text_kind kind = Format::kind();
    const long long trows = Format::text_rows(rows);
    const unsigned long long bytes = Format::text_bytes(width, rows);
    const trt_text_split split = trt_text_split_of((unsigned long long)out, bytes);
    if (wave == 0)
    {
        const long long lone = trt_text_lone_byte(&split, lane);
        if (lone >= 0)
            out[lone] = (unsigned char)Format::lone_value(lone, bytes);
    }
    const unsigned long long first = trt_text_lane_word(kind, wave, 0, 0);
    if (first >= split.words) // the whole wave: a frame of a batch whose alignment needs a wave less than the grid has
        return;
    const trt_text_at from = trt_text_locate(kind, split.head + 4 * first, width, trows);
    const typename Format::held mine = Format::hold(from, lane, width, rows, width_magic, fetch);
    unsigned char *const words = out + split.head;
#pragma unroll
    for (int j = 0; j < Format::turns; j++)
    {
        const unsigned long long k = trt_text_lane_word(kind, wave, lane, j);
        trt_text_at at[4]; // the word's four bytes; other[b]: byte b stands in another cell than byte 0
        unsigned other[4] = {0u};
        at[0] = trt_text_advance(kind, &from, 4u * (unsigned)(64 * j + lane), width, trows, row_magic);
#pragma unroll
        for (int b = 1; b < 4; b++)
        {
            at[b] = at[b - 1];
            other[b] = other[b - 1] | (unsigned)trt_text_step(kind, &at[b], width, trows);
        }
        const typename Format::seen shown = Format::colours(at[0], at[3], from, mine, width);
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; b++)
            word |= Format::byte(at[b], rows, shown, other[b]) << (8 * b);
        if (k < split.words)
            *reinterpret_cast<unsigned *>(words + 4 * k) = word; // (out + head) is 4-aligned
    }
}

// The full text: a lane holds ONE pixel in one register, `pixel_rgb(p)`: r | g << 8 | b << 16 of pixel p < width * rows.  A word shows
// at most two pixels (trt_ansi.h), that of its first byte and that of its last: two reads of the one register.
struct ansi_text
{
    static constexpr int turns = TRT_ANSI_WAVE_WORDS / 64;
    using held = unsigned;
    struct seen
    {
        unsigned first, last;
    };
    static __device__ __forceinline__ trt_text_kind kind() { return trt_ansi_kind(); }
    static __device__ __forceinline__ long long text_rows(int rows) { return trt_ansi_text_rows(rows); }
    static __device__ __forceinline__ unsigned long long text_bytes(int width, int rows) { return trt_ansi_text_bytes(width, rows); }
    static __device__ __forceinline__ unsigned lone_value(long long position, unsigned long long bytes) { return trt_ansi_lone_value(position, bytes); }

    template <class Fetch>
    static __device__ __forceinline__ held hold(const trt_text_at &from, int lane, int width, int rows, unsigned, Fetch pixel_rgb)
    {
        const long long pixels = (long long)width * rows, p0 = trt_text_cell(&from, width);
        return p0 + lane < pixels ? pixel_rgb(p0 + lane) : 0u;
    }
    static __device__ __forceinline__ seen colours(const trt_text_at &at, const trt_text_at &last, const trt_text_at &from, held mine, int width)
    {
        const long long p0 = trt_text_cell(&from, width);
        seen shown;
        shown.first = (unsigned)__shfl((int)mine, (int)(trt_text_cell(&at, width) - p0) & 63);
        shown.last = (unsigned)__shfl((int)mine, (int)(trt_text_cell(&last, width) - p0) & 63);
        return shown;
    }
    static __device__ __forceinline__ unsigned byte(const trt_text_at &at, int rows, seen shown, unsigned other)
    {
        return trt_ansi_byte(&at, rows, other ? shown.last : shown.first);
    }
};

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

// the two pixels of a half-block cell, formed TOGETHER (trt_ansi_half.hpp, trt_ansi256.hpp)
struct ansi_half_pair
{
    unsigned upper, lower; // r | g << 8 | b << 16 each
};

// pixels p and q of a frame's scratch (as ansi_pixel_of_samples forms one): each sum from 0.0 in sample order, the two side by side
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

// What a Format's hold() is given as `fetch`, from either source: (p) forms pixel p < width * rows as r | g << 8 | b << 16 for the formats
// whose cell is one pixel, (p, q) the pixels p and q together for the half-block formats.
// ... from ONE frame's scratch: the ordered mean and the emitter's cast
struct pixels_of_samples
{
    const double *samples;
    long values;
    int spp;
    double inv_spp;
    __device__ __forceinline__ unsigned operator()(long long p) const { return ansi_pixel_of_samples(samples, values, spp, inv_spp, p); }
    __device__ __forceinline__ ansi_half_pair operator()(long long p, long long q) const { return ansi_half_pixels_of_samples(samples, values, spp, inv_spp, p, q); }
};

// ... from a frame that exists as RGB8 bytes rgb[p * 3 + channel]
struct pixels_of_rgb8
{
    const unsigned char *rgb;
    __device__ __forceinline__ unsigned operator()(long long p) const
    {
        const unsigned char *px = rgb + 3 * p;
        return (unsigned)px[0] | (unsigned)px[1] << 8 | (unsigned)px[2] << 16;
    }
    __device__ __forceinline__ ansi_half_pair operator()(long long p, long long q) const
    {
        ansi_half_pair both;
        both.upper = (*this)(p);
        both.lower = (*this)(q);
        return both;
    }
};

// Every kernel that writes a whole text has ONE of two argument lists, whatever its format reads of it (the full-cell formats ignore
// width_magic, the kitty image, trt_kitty.hpp, both magics): the host launches them through these types (trt_render.hip).
using TextMeanKernel = void (*)(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic, unsigned width_magic, int spp, double inv_spp,
                                unsigned int *queue, unsigned grid, unsigned waves_per_group, unsigned shift);
using TextFromRgb8Kernel = void (*)(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic, unsigned width_magic);

// The ordered mean, the emitter's cast and the Format's text in ONE pass, as the last kernel of a launch in reduce_samples_kernel's
// place: blockIdx.y is the frame, and it leaves the queue ready in the same way.  Frame b's text starts at out + b * Format::text_bytes,
// aligned to nothing in general: every frame has a head and a tail of its own.  A single frame's grid has trt_text_waves(words of the
// text at `out`) waves; that of several frames the most waves an alignment needs (a frame's spare wave finds nothing to do).
template <class Format>
__global__ __launch_bounds__(256) void reduce_samples_text_kernel(const double *samples, unsigned char *out, int width, int rows, unsigned row_magic,
                                                                  unsigned width_magic, int spp, double inv_spp, unsigned int *queue, unsigned grid,
                                                                  unsigned waves_per_group, unsigned shift)
{
    arm_queue(queue, grid, waves_per_group, shift);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long values = (long)width * rows * 3;
    text_write<Format>(out + (size_t)blockIdx.y * (size_t)Format::text_bytes(width, rows), width, rows, row_magic, width_magic, t >> 6, (int)(t & 63),
                       pixels_of_samples{samples + (size_t)blockIdx.y * (size_t)spp * (size_t)values, values, spp, inv_spp});
}

// The formatting alone, of a frame that exists as RGB8 bytes (the ..._from_rgb8_device entries; the reference-order kernel's frames,
// which have no scratch)
template <class Format>
__global__ __launch_bounds__(256) void text_from_rgb8_kernel(const unsigned char *rgb, unsigned char *out, int width, int rows, unsigned row_magic, unsigned width_magic)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    text_write<Format>(out, width, rows, row_magic, width_magic, t >> 6, (int)(t & 63), pixels_of_rgb8{rgb});
}

#endif // TRT_UNIT_RENDER

} // namespace trt
