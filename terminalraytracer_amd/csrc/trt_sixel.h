/*
 * trt_sixel.h -- the format of a frame as a DEC SIXEL image, with its position map and its lane map (host + device, plain C).
 *
 * The kitty image of trt_kitty.h gives true pixels to the terminals that speak that protocol.  xterm, foot, mlterm, Windows Terminal, VS
 * Code's terminal, contour and tmux built with sixel take SIXEL and nothing else: a picture in bands of six pixel rows, a band drawn one
 * colour register at a time, every data character six pixels of one column -- bit j set: the pixel of the band's row j has this colour.
 * For a screen of `width` x `rows` owned rows, in local row order as the other texts, in order,
 *
 *      "\033[0;0H"                               6 bytes   cursor home, as every other text
 *      "\033P0;1;0q"                             8 bytes   DCS, P2 = 1: a 0 bit leaves its pixel alone
 *      "\"1;1;WWWWW;RRRRR"                      16 bytes   raster attributes, width and rows, five zero-padded digits each
 *      240 x "#NNN;2;PPP;PPP;PPP"             4320 bytes   colour register NNN = 016..255, ascending: the xterm palette's entry NNN
 *                                                          (trt_xterm256.h) in RGB per cent, PPP = (100 v + 127) / 255 in integers, three
 *                                                          zero-padded digits (levels 0 37 53 69 84 100; greys 3 7 11 ... 93)
 *      per band b = 0 .. ceil(rows / 6) - 1, six pixel rows each (the last has fewer), and in it
 *        per palette index n, ASCENDING, that at least one pixel of the band has (trt_xterm256_index of its emitter bytes), a COLOUR ROW:
 *          "#NNN"                                4 bytes
 *          width data characters                 63 + the sum over j of (the pixel of row 6 b + j in this column has index n) << j;
 *                                                rows >= `rows` give 0
 *          T - 1 times "$", then one more byte   "-" behind the LAST colour of every band but the last band, "$" everywhere else
 *      "\033\\"                                  2 bytes
 *
 * T = 1 + ((-(width + 1)) mod 4) is 1..4, so a colour row is L = 4 + width + T bytes, a multiple of 4: a repeated "$" is a repeated
 * graphics carriage return and changes nothing, and that padding, not a "!" repeat, keeps every colour row at one length and the data
 * words of a frame at ONE alignment.  The text has 4352 + L * (the sum over the bands of k_b) bytes, k_b the distinct indices of band b:
 * its length depends on the picture.  No NUL, no newline.  trt_sixel_capacity_bytes is 4352 + L * the sum of min(240, width * rows of band b),
 * in 64 bits.  width and rows are at most 99999 each (five digits); above, lengths are 0.  trt_emitter_sixel_rgb8
 * (csrc/host/trt_emit.c) is the sequential statement.
 *
 * NO TERMINAL HAS SHOWN THIS PICTURE.  The format is written from memory of DEC's description; no terminal and no documentation of it were
 * at hand where this was built, and the tests hold the text against a structural reader (tests/sixel_support.py), not a terminal.
 * Registers up to 255 need a terminal with 256 colour registers: xterm as a VT340 defaults to 16 and needs `numColorRegisters: 256`.  A
 * per-cent palette cannot say 95 or 135 exactly, so the colours are within 1/100 of the xterm palette's.
 *
 * Out of scope: "!" run-length repeats; dithering; any palette other than the 240 fixed entries; a delta form; batch forms; a refraction
 * form; tmux pass-through.
 *
 * The device route (trt_sixel.hpp) is the delta text's scheme, three kernels in stream order:
 *   measure   a workgroup per band ORs the indices of the band's pixels into a 240-bit mask (bit i: index 16 + i), 8 words, and counts it
 *   offsets   ONE workgroup scans the bands' counts exclusively into the index of every band's first colour row, stores the length, and
 *             writes the 4350 bytes in front of the first colour row (trt_sixel_prologue_byte) and the two behind the last
 *   write     a workgroup per band and tile of TRT_SIXEL_BLOCK slots; see the lane map
 *
 * The position map.  Colour row q (counted through the text) starts at 4350 + L q; within it offset o is byte o of "#NNN" (o < 4), the
 * data character of column o - 4 (o < 4 + width) or a terminator byte: trt_sixel_row_literal, and trt_sixel_lane_word for the data.
 *
 * The lane map.  4350 + L q is the same modulo 4 for every q, so every colour row of a frame has ONE split (trt_text_split_of of the first
 * row's address and L): `head` bytes in front of the first 4-aligned address, L / 4 or L / 4 - 1 aligned words, `tail` bytes.  A SLOT is
 * what one thread stores of every colour row of its band: slot s covers the offsets [4 s - lead, 4 s - lead + 4) that lie in [0, L),
 * lead = (4 - head) mod 4 -- slot 0 the head where there is one, the last slot the tail, every other an aligned word; a row has
 * trt_sixel_slots of them.  A slot shows at most four adjacent columns, the SAME for every colour of the band: the thread forms their 6 x 4
 * palette indices once (trt_sixel_lane_of: six registers, a byte an index, 0 where there is no pixel -- no index is below 16), then walks
 * the band's mask in ascending order -- the walk is the same in every lane of a wave -- and stores, per colour, one aligned word
 * (trt_sixel_lane_word), or the bytes of a partial slot one by one.  Every byte of a colour row belongs to exactly one slot.
 */
#ifndef TRT_SIXEL_H
#define TRT_SIXEL_H

#include "trt_text_map.h"
#include "trt_xterm256.h"

#define TRT_SIXEL_HD TRT_TEXT_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_SIXEL_UNROLL _Pragma("unroll") /* a lane's indices are registers only where every loop over them is unrolled */
#else
#define TRT_SIXEL_UNROLL /* the host compiler is left to itself */
#endif

#define TRT_SIXEL_MAX 99999
#define TRT_SIXEL_COLOURS 240   /* registers 16 .. 255 */
#define TRT_SIXEL_MASK_WORDS 8  /* 32 bits each: bit i of the mask is index 16 + i; the 16 highest bits stay 0 */
#define TRT_SIXEL_BAND 6        /* pixel rows of a band */
#define TRT_SIXEL_HOME TRT_TEXT_HOME
#define TRT_SIXEL_DCS 8         /* strlen("\033P0;1;0q") */
#define TRT_SIXEL_RASTER 16     /* strlen("\"1;1;WWWWW;RRRRR") */
#define TRT_SIXEL_DEFINITION 18 /* strlen("#NNN;2;PPP;PPP;PPP") */
#define TRT_SIXEL_PROLOGUE (TRT_SIXEL_HOME + TRT_SIXEL_DCS + TRT_SIXEL_RASTER + TRT_SIXEL_COLOURS * TRT_SIXEL_DEFINITION) /* 4350 */
#define TRT_SIXEL_END 2         /* strlen("\033\\") */
#define TRT_SIXEL_FIXED (TRT_SIXEL_PROLOGUE + TRT_SIXEL_END) /* 4352 */
#define TRT_SIXEL_BLOCK 256       /* threads of a workgroup of the measure and write kernels; a write workgroup's slots */
#define TRT_SIXEL_SCAN_BLOCK 1024 /* threads of the one workgroup that scans the bands' counts */

TRT_SIXEL_HD int trt_sixel_size_ok(int width, long long rows) { return width > 0 && rows > 0 && width <= TRT_SIXEL_MAX && rows <= TRT_SIXEL_MAX; }

/* T: the bytes that end a colour row, 1..4 */
TRT_SIXEL_HD int trt_sixel_pad(int width) { return 1 + ((4 - (width + 1) % 4) & 3); }

/* L: the bytes of a colour row, a multiple of 4 */
TRT_SIXEL_HD int trt_sixel_row_bytes(int width) { return 4 + width + trt_sixel_pad(width); }

TRT_SIXEL_HD int trt_sixel_bands(int rows) { return (rows + TRT_SIXEL_BAND - 1) / TRT_SIXEL_BAND; }

/* pixel rows of band `band`: six, fewer in the last */
TRT_SIXEL_HD int trt_sixel_band_rows(int rows, int band)
{
    const int left = rows - TRT_SIXEL_BAND * band;
    return left < TRT_SIXEL_BAND ? left : TRT_SIXEL_BAND;
}

/* the length of a text of `colour_rows` colour rows */
TRT_SIXEL_HD unsigned long long trt_sixel_text_bytes(int width, unsigned long long colour_rows)
{
    return TRT_SIXEL_FIXED + (unsigned long long)trt_sixel_row_bytes(width) * colour_rows;
}

/* the most colour rows a frame has: min(240, the band's pixels) per band */
TRT_SIXEL_HD unsigned long long trt_sixel_most_colour_rows(int width, int rows)
{
    const unsigned long long whole = (unsigned long long)(rows / TRT_SIXEL_BAND), last = (unsigned long long)(rows % TRT_SIXEL_BAND);
    const unsigned long long in_whole = (unsigned long long)width * TRT_SIXEL_BAND, in_last = (unsigned long long)width * last;
    return whole * (in_whole < TRT_SIXEL_COLOURS ? in_whole : TRT_SIXEL_COLOURS) + (in_last < TRT_SIXEL_COLOURS ? in_last : TRT_SIXEL_COLOURS);
}

/* room for any text of the size; 0 for a screen that has none: a size that is not positive or above five digits */
TRT_SIXEL_HD unsigned long long trt_sixel_capacity_bytes(int width, long long rows)
{
    if (!trt_sixel_size_ok(width, rows))
        return 0;
    return trt_sixel_text_bytes(width, trt_sixel_most_colour_rows(width, (int)rows));
}

/* ---- the palette ---- */

/* channel 0..2 (R, G, B) of the xterm palette's entry n = 16..255, a byte */
TRT_SIXEL_HD unsigned trt_sixel_palette_byte(unsigned n, int channel)
{
    if (n >= TRT_XTERM256_GREYS)
        return 8u + 10u * (n - TRT_XTERM256_GREYS);
    const unsigned c = n - TRT_XTERM256_FIRST, level = channel == 0 ? c / 36u : channel == 1 ? c / 6u % 6u : c % 6u;
    return trt_xterm256_level_value(level);
}

/* a byte in per cent, rounded */
TRT_SIXEL_HD unsigned trt_sixel_percent(unsigned v) { return (100u * v + 127u) / 255u; }

/* digit k = 0..2 of v < 1000 as three zero-padded digits, a character */
TRT_SIXEL_HD unsigned trt_sixel_digit3(unsigned v, int k) { return '0' + (k == 0 ? v / 100u : k == 1 ? v / 10u % 10u : v % 10u); }

/* digit k = 0..4 of v < 100000 as five zero-padded digits, a character */
TRT_SIXEL_HD unsigned trt_sixel_digit5(unsigned v, int k)
{
    const unsigned p = k == 0 ? 10000u : k == 1 ? 1000u : k == 2 ? 100u : k == 3 ? 10u : 1u;
    return '0' + v / p % 10u;
}

/* ---- the position map ---- */

/* byte `at` < TRT_SIXEL_PROLOGUE of the text: what stands in front of the first colour row */
TRT_SIXEL_HD unsigned trt_sixel_prologue_byte(unsigned at, int width, int rows)
{
    const unsigned long long home = TRT_TEXT_PACK8('\033', '[', '0', ';', '0', 'H', 0, 0), dcs = TRT_TEXT_PACK8('\033', 'P', '0', ';', '1', ';', '0', 'q');
    if (at < TRT_SIXEL_HOME)
        return (unsigned)(home >> (8 * at)) & 0xffu;
    at -= TRT_SIXEL_HOME;
    if (at < TRT_SIXEL_DCS)
        return (unsigned)(dcs >> (8 * at)) & 0xffu;
    at -= TRT_SIXEL_DCS;
    if (at < TRT_SIXEL_RASTER) /* "1;1;WWWWW;RRRRR */
        return at == 0 ? '"' : at == 1 || at == 3 ? '1' : at == 2 || at == 4 || at == 10 ? ';' : at < 10 ? trt_sixel_digit5((unsigned)width, (int)at - 5) : trt_sixel_digit5((unsigned)rows, (int)at - 11);
    at -= TRT_SIXEL_RASTER;
    const unsigned n = TRT_XTERM256_FIRST + at / TRT_SIXEL_DEFINITION, c = at % TRT_SIXEL_DEFINITION; /* #NNN;2;PPP;PPP;PPP */
    if (c == 0)
        return '#';
    if (c < 4)
        return trt_sixel_digit3(n, (int)c - 1);
    if (c == 5)
        return '2';
    if (c == 4 || c == 6 || c == 10 || c == 14)
        return ';';
    const int channel = (int)(c - 7) / 4;
    return trt_sixel_digit3(trt_sixel_percent(trt_sixel_palette_byte(n, channel)), (int)(c - 7) % 4);
}

/* byte e = 0, 1 behind the last colour row */
TRT_SIXEL_HD unsigned trt_sixel_end_byte(unsigned e) { return e ? '\\' : '\033'; }

/* byte `o` < L of a colour row of index n that is not a data character: o < 4 or o >= 4 + width; `dash`: the last colour row of a band that
 * is not the last band */
TRT_SIXEL_HD unsigned trt_sixel_row_literal(int o, unsigned n, int width, int dash)
{
    if (o == 0)
        return '#';
    if (o < 4)
        return trt_sixel_digit3(n, o - 1);
    return dash && o == trt_sixel_row_bytes(width) - 1 ? '-' : '$';
}

/* ---- the masks ---- */

TRT_SIXEL_HD void trt_sixel_mask_set(unsigned *mask, unsigned n) { mask[(n - TRT_XTERM256_FIRST) >> 5] |= 1u << ((n - TRT_XTERM256_FIRST) & 31u); }

/* the index of bit `bit` of mask word `word` */
TRT_SIXEL_HD unsigned trt_sixel_mask_index(int word, int bit) { return TRT_XTERM256_FIRST + 32u * (unsigned)word + (unsigned)bit; }

/* ---- the lane map ---- */

/* the split every colour row of the text at `address` has */
TRT_SIXEL_HD trt_text_split trt_sixel_row_split(unsigned long long address, int width)
{
    return trt_text_split_of(address + TRT_SIXEL_PROLOGUE, (unsigned long long)trt_sixel_row_bytes(width));
}

/* slots of a colour row: its words, and one each for a head and a tail */
TRT_SIXEL_HD unsigned trt_sixel_slots(const trt_text_split *split) { return (unsigned)split->words + (split->head != 0) + (split->tail != 0); }

/* the offset in its colour row of slot s's first byte, negative where the slot is the head: 4 s - lead */
TRT_SIXEL_HD int trt_sixel_slot_first(const trt_text_split *split, unsigned s) { return 4 * (int)s - (int)((4u - split->head) & 3u); }

typedef struct
{
    unsigned index[TRT_SIXEL_BAND]; /* per row of the band: the palette indices of the slot's four offsets, a byte each, 0 where the offset shows no pixel */
} trt_sixel_lane;

/* what a thread keeps of its slot: the indices of the pixels at the offsets first .. first + 3 of band `band`'s colour rows, from the frame's
 * RGB8 bytes rgb[(row * width + column) * 3 + channel] */
TRT_SIXEL_HD trt_sixel_lane trt_sixel_lane_of(const unsigned char *rgb, int width, int rows, int band, int first)
{
    trt_sixel_lane lane;
    const int band_rows = trt_sixel_band_rows(rows, band);
    TRT_SIXEL_UNROLL
    for (int j = 0; j < TRT_SIXEL_BAND; j++)
    {
        unsigned four = 0;
        TRT_SIXEL_UNROLL
        for (int i = 0; i < 4; i++)
        {
            const int column = first + i - 4;
            if (j < band_rows && column >= 0 && column < width)
            {
                const unsigned char *px = rgb + 3 * ((long long)(TRT_SIXEL_BAND * band + j) * width + column);
                four |= trt_xterm256_index(px[0], px[1], px[2]) << (8 * i);
            }
        }
        lane.index[j] = four;
    }
    return lane;
}

/* the four bytes at the offsets first .. first + 3 of the colour row of index n, the first in the low byte; 0 where an offset is outside
 * the row */
TRT_SIXEL_HD unsigned trt_sixel_lane_word(const trt_sixel_lane *lane, int first, unsigned n, int width, int dash)
{
    const int row_bytes = trt_sixel_row_bytes(width);
    unsigned word = 0;
    TRT_SIXEL_UNROLL
    for (int i = 0; i < 4; i++)
    {
        const int o = first + i;
        unsigned byte = 0;
        if (o >= 4 && o < 4 + width)
        {
            byte = 63u;
            TRT_SIXEL_UNROLL
            for (int j = 0; j < TRT_SIXEL_BAND; j++)
                byte += (unsigned)(((lane->index[j] >> (8 * i)) & 0xffu) == n) << j;
        }
        else if (o >= 0 && o < row_bytes)
            byte = trt_sixel_row_literal(o, n, width, dash);
        word |= byte << (8 * i);
    }
    return word;
}

#endif /* TRT_SIXEL_H */
