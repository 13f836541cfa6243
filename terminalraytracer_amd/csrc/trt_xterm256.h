/*
 * trt_xterm256.h -- a pixel's colour in the xterm 256-colour palette (host + device, plain C).
 *
 * Terminals without 24-bit SGR colour take "\033[48;5;Nm", N an entry of a palette of 256.  Entries 0..15 are the terminal's own to
 * theme and are NEVER produced here; the 240 others are fixed numbers:
 *
 *      16 + 36 i + 6 j + k    the colour (L[i], L[j], L[k]), L = {0, 95, 135, 175, 215, 255}       the 6 x 6 x 6 cube
 *      232 + k                the grey 8 + 10 k, k = 0..23                                         the grey ramp
 *
 * THE RULE: of these 240 the entry with the least squared Euclidean distance in RGB bytes, ties to the LOWEST index.  That is the
 * search trt_xterm256_index_search (csrc/host/trt_emit.c) carries out; trt_xterm256_index below is a closed form of it, equal to it
 * on all 2^24 colours (tests/xterm256_check.c walks them):
 *
 *   - the cube.  The distance is a sum over channels, so the nearest cube colour is the nearest level per channel.  The midpoints of
 *     neighbouring levels are 47.5, 115, 155, 195, 235: level 0 below 48, else one more for every midpoint EXCEEDED -- a byte on a
 *     midpoint takes the lower level, which is the lower index, in every channel at once.
 *   - the ramp.  The sum of (c - v)^2 over the three channels is least for the grey v nearest to their mean S / 3, S = r + g + b: k is
 *     (S - 24) / 30 rounded to the nearest, a half (S = 30 k + 39) DOWN to the lower index: k = (S - 10) / 30 in integers, 0 for
 *     S <= 39, 23 at the most.
 *   - every ramp index is above every cube index, so the grey wins only where it is STRICTLY nearer.
 *
 * There is NO DITHERING: an index is a function of the pixel's three emitter bytes alone, not of its place or its neighbours, so that
 * a still scene gives a still text and the device's map can be held against the host's on every colour.
 */
#ifndef TRT_XTERM256_H
#define TRT_XTERM256_H

#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_XTERM256_HD __host__ __device__ __forceinline__
#else
#define TRT_XTERM256_HD static inline __attribute__((always_inline))
#endif

#define TRT_XTERM256_FIRST 16  /* the lowest index produced: the cube's black */
#define TRT_XTERM256_GREYS 232 /* the ramp's first index */
#define TRT_XTERM256_BLACK 16  /* what stands where a frame has no pixel (behind the last row of an odd half-block frame) */

/* the cube level 0..5 nearest to a byte, the lower of two that are equally near */
TRT_XTERM256_HD unsigned trt_xterm256_level(unsigned c)
{
    return (unsigned)(c >= 48u) + (unsigned)(c > 115u) + (unsigned)(c > 155u) + (unsigned)(c > 195u) + (unsigned)(c > 235u);
}

/* L[level]: 0, 95, 135, 175, 215, 255 */
TRT_XTERM256_HD unsigned trt_xterm256_level_value(unsigned level) { return level ? 55u + 40u * level : 0u; }

/* the palette entry 16..255 of the colour (r, g, b), bytes each */
TRT_XTERM256_HD unsigned trt_xterm256_index(unsigned r, unsigned g, unsigned b)
{
    const unsigned i = trt_xterm256_level(r), j = trt_xterm256_level(g), k = trt_xterm256_level(b);
    const int dr = (int)r - (int)trt_xterm256_level_value(i), dg = (int)g - (int)trt_xterm256_level_value(j), db = (int)b - (int)trt_xterm256_level_value(k);
    const unsigned sum = r + g + b, ramp = sum <= 39u ? 0u : (sum - 10u) / 30u, grey = ramp > 23u ? 23u : ramp;
    const int v = 8 + 10 * (int)grey, er = (int)r - v, eg = (int)g - v, eb = (int)b - v;
    const int cube_distance = dr * dr + dg * dg + db * db, grey_distance = er * er + eg * eg + eb * eb;
    return grey_distance < cube_distance ? TRT_XTERM256_GREYS + grey : TRT_XTERM256_FIRST + 36u * i + 6u * j + k;
}

/* the same of a pixel packed as the texts' lanes hold one: r | g << 8 | b << 16 */
TRT_XTERM256_HD unsigned trt_xterm256_index_of(unsigned rgb) { return trt_xterm256_index(rgb & 0xffu, (rgb >> 8) & 0xffu, (rgb >> 16) & 0xffu); }

#endif /* TRT_XTERM256_H */
