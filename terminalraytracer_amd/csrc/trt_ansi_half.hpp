// trt_ansi_half.hpp -- the frame as the terminal's HALF-BLOCK text, written on the device, two pixel rows per line of text.
// trt_text_map.h holds the position map and the lane map, trt_ansi_half.h the format, trt_ansi.hpp the wave that carries them out
// (text_write), the fetches and the two kernels (reduce_samples_text_kernel, text_from_rgb8_kernel); this file says what a lane of that
// wave holds of a half-block cell and how a word fetches it.
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

#endif // TRT_UNIT_RENDER

} // namespace trt
