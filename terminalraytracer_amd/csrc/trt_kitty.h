/*
 * trt_kitty.h -- the format of a frame as a KITTY GRAPHICS-PROTOCOL image, with its position map and its lane map (host + device, plain C).
 *
 * The texts of trt_ansi.h and trt_ansi_half.h paint a pixel with character cells, 25 and 19.5 bytes a pixel.  A terminal that speaks the
 * kitty graphics protocol takes true pixels, as base64 of RGB bytes inside APC escape sequences: three bytes are exactly four base64
 * characters, so a pixel is ONE 32-bit word of text and no padding ever occurs.  For a screen of `width` x `rows` owned rows, P = width *
 * rows pixels in local row order, K = ceil(P / 1024) chunks, in order,
 *
 *      "\033[0;0H"                                                        6 bytes, the home prefix (as every whole text)
 *      chunk 0:   "\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=WWWWW,v=RRRRR,m=M;"  48 bytes: WWWWW = width, RRRRR = rows, five zero-padded digits each
 *                 the payload of chunk 0
 *                 "\033\\"                                                2 bytes
 *      chunk c>0: "\033_Gm=0M;"                                           8 bytes
 *                 the payload of chunk c
 *                 "\033\\"                                                2 bytes
 *
 * The payload of chunk c holds the pixels 1024 c up to min(P, 1024 (c + 1)), four characters each: RFC 4648 base64, standard alphabet, of
 * the emitter's bytes R, G, B ((int)(colour*255), trt_render_device_rgb8's).  Every chunk but the last carries 4096 characters, the
 * protocol's limit per escape.  M is 1 in every chunk but the last and 0 in the last.  No '=', no newline, no NUL:
 * trt_kitty_text_bytes = 4 P + 10 K + 46.  width and rows are at most 99999 (five digits); above, the text has no length.
 * trt_emitter_kitty_rgb8 (csrc/host/trt_emit.c) is the sequential statement.
 *
 * The keys: a=T transmit and display; f=24 RGB; i=1,p=1 image and placement id, so that re-sending replaces the picture in place; q=2 the
 * terminal answers nothing; C=1 the cursor stays; s, v the picture's size; m more chunks follow.
 * NO TERMINAL HAS YET SHOWN THIS PICTURE.  The key list is written from memory of the protocol; no terminal and no documentation of it were
 * at hand when this was built, and what stands in for a terminal is a structural reader in the tests (tests/kitty_support.py).  For that
 * reason the 48-byte header is ONE literal, TRT_KITTY_HEADER, with the places of its digits beside it: whoever tries it on a terminal and
 * finds a key wrong changes it in this one place (and the same literal in trt_emit.c, which on purpose does not include this file).
 * The later chunks' header is 8 bytes, its M zero-padded to two digits as s and v are padded: the 10 bytes between two payloads make the
 * chunk stride 4106 = 2 mod 4 and the length's 10 K.
 *
 * Out of scope: delta / animation frames (a=f); compression (o=z); shared-memory transmission; a refraction form; tmux pass-through;
 * anything in trt_dist_* (rank 0 formats a gathered RGB8 frame with trt_kitty_from_rgb8_device).
 *
 * The position map.  trt_text_map.h's does not fit -- the prefix is 54 bytes, a "row" is 1024 cells whatever the width, the 10 bytes
 * between two payloads are longer than a cell, the last row is short, and the M before the last payload differs -- so this header has its
 * own.  A position is a trt_kitty_at: the chunk, and the byte counted from the chunk's first payload character, negative in front of it.
 * trt_kitty_locate finds it with a 64-bit division by the constant stride, once per WAVE; trt_kitty_advance finds the position d < 4106
 * bytes behind with a compare.  Pixels and chunks are 32-bit (P < 2^31).
 *
 * The lane map.  As trt_text_map.h's: `head` bytes in front of the first 4-aligned address, `words` aligned words, `tail` < 4 bytes
 * (trt_text_split_of); wave g owns the 64 words from 64 g, lane l word 64 g + l (trt_text_lane_word): 256 consecutive bytes per store
 * instruction.  The head lies in the home prefix (3 < 6) and wave 0's lanes 0..2 store it.  The tail does NOT lie in constants -- the text
 * ends in 2 bytes, a tail of 3 shows the last pixel's last character -- so it counts as one more, partial, word: slot `words`, whose lane
 * forms it like any word and stores its `tail` bytes one by one.
 * A wave's 256 bytes touch at most 65 pixels (TRT_KITTY_SPAN_PIXELS): 64 when the payload is 4-aligned at the wave's first byte, the
 * rest of one, 63 whole ones and the beginning of another when it is not.  The stride is 2 mod 4, so the alignment changes from chunk to
 * chunk.  Lane l forms pixel p0 + l, p0 the first pixel at or behind the wave's first byte, for l < count, the pixels the wave's bytes
 * show; when there are 65, lane 63 forms p0 + 64 too (the EXTRA pixel, which is the next wave's p0).  So a pixel is formed by at most two
 * waves and a wave forms at most one pixel that the wave before it has formed.  A word shows at most two pixels, and they are
 * neighbours: 10 bytes lie between two payloads.
 */
#ifndef TRT_KITTY_H
#define TRT_KITTY_H

#include "trt_text_map.h"

#define TRT_KITTY_HD TRT_TEXT_HD

#define TRT_KITTY_HOME TRT_TEXT_HOME
/* THE header, one literal: untested on a terminal.  Digits are added to the '0's at WIDTH_AT, ROWS_AT (five each) and MORE_AT (one). */
#define TRT_KITTY_HEADER "\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=00000,v=00000,m=0;"
#define TRT_KITTY_HEADER_BYTES 48
#define TRT_KITTY_WIDTH_AT 30
#define TRT_KITTY_ROWS_AT 38
#define TRT_KITTY_MORE_AT 46
#define TRT_KITTY_CHUNK_HEADER "\033_Gm=00;"
#define TRT_KITTY_CHUNK_HEADER_BYTES 8
#define TRT_KITTY_CHUNK_MORE_AT 6
#define TRT_KITTY_END 2 /* strlen("\033\\") */
#define TRT_KITTY_CHUNK_PIXELS 1024
#define TRT_KITTY_PAYLOAD (4 * TRT_KITTY_CHUNK_PIXELS)
#define TRT_KITTY_STRIDE (TRT_KITTY_CHUNK_HEADER_BYTES + TRT_KITTY_PAYLOAD + TRT_KITTY_END) /* 4106: from one payload's first character to the next one's */
#define TRT_KITTY_FIRST (TRT_KITTY_HOME + TRT_KITTY_HEADER_BYTES)                           /* 54: the first payload's position */
#define TRT_KITTY_MAX 99999
#define TRT_KITTY_WAVE_WORDS 64
#define TRT_KITTY_SPAN (4 * TRT_KITTY_WAVE_WORDS)
#define TRT_KITTY_SPAN_PIXELS (TRT_KITTY_WAVE_WORDS + 1)

/* for trt_text_waves and trt_text_lane_word: a wave's words */
TRT_KITTY_HD trt_text_kind trt_kitty_kind(void)
{
    const trt_text_kind kind = {4, 0, TRT_KITTY_WAVE_WORDS, 0};
    return kind;
}

typedef struct
{
    int pixels; /* P */
    int chunks; /* K */
} trt_kitty_shape;

/* length of the text; 0 for a screen that has none: a size that is not positive or above five digits */
TRT_KITTY_HD unsigned long long trt_kitty_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0 || width > TRT_KITTY_MAX || rows > TRT_KITTY_MAX)
        return 0;
    const unsigned long long pixels = (unsigned long long)width * (unsigned long long)rows;
    return 4 * pixels + 10 * ((pixels + TRT_KITTY_CHUNK_PIXELS - 1) / TRT_KITTY_CHUNK_PIXELS) + 46;
}

/* of a screen that has a text and fewer than 2^31 pixels */
TRT_KITTY_HD trt_kitty_shape trt_kitty_shape_of(int width, int rows)
{
    trt_kitty_shape s;
    s.pixels = width * rows;
    s.chunks = (int)(((unsigned)s.pixels + TRT_KITTY_CHUNK_PIXELS - 1) / TRT_KITTY_CHUNK_PIXELS);
    return s;
}

/* pixels of chunk `chunk`: 1024, fewer in the last, none behind it */
TRT_KITTY_HD int trt_kitty_chunk_pixels(const trt_kitty_shape *s, int chunk)
{
    return chunk < s->chunks - 1 ? TRT_KITTY_CHUNK_PIXELS : chunk == s->chunks - 1 ? s->pixels - TRT_KITTY_CHUNK_PIXELS * (s->chunks - 1) : 0;
}

/* the base64 character of a sextet: compares and adds */
TRT_KITTY_HD unsigned trt_kitty_base64(unsigned v)
{
    return v + 65u + (v >= 26u ? 6u : 0u) - (v >= 52u ? 75u : 0u) - (v >= 62u ? 15u : 0u) + (v >= 63u ? 3u : 0u);
}

/* the four characters of the pixel rgb = r | g << 8 | b << 16, the first in the low byte: what a lane keeps */
TRT_KITTY_HD unsigned trt_kitty_chars(unsigned rgb)
{
    const unsigned n = (rgb & 0xffu) << 16 | (rgb & 0xff00u) | (rgb >> 16 & 0xffu);
    return trt_kitty_base64(n >> 18) | trt_kitty_base64(n >> 12 & 63u) << 8 | trt_kitty_base64(n >> 6 & 63u) << 16 | trt_kitty_base64(n & 63u) << 24;
}

/* ---- the position map ---- */

typedef struct
{
    int chunk; /* the chunk; what stands in front of a payload, the home prefix too, counts to it.  >= K: behind the text */
    int r;     /* byte counted from the chunk's first payload character: -54 .. -49 the home prefix, -48 .. -1 the first header (chunk 0); -8 .. -1 a
                  later chunk's header; 0 .. 4 n - 1 the payload of the chunk's n pixels; 4 n, 4 n + 1 the terminator; behind that in the last chunk:
                  behind the text */
} trt_kitty_at;

enum
{
    TRT_KITTY_IN_HOME,
    TRT_KITTY_IN_HEADER,       /* the first chunk's */
    TRT_KITTY_IN_CHUNK_HEADER, /* a later chunk's */
    TRT_KITTY_IN_PAYLOAD,      /* character r & 3 of pixel 1024 chunk + (r >> 2) */
    TRT_KITTY_IN_END,          /* the terminator */
    TRT_KITTY_BEHIND           /* behind the last chunk */
};

TRT_KITTY_HD int trt_kitty_what(const trt_kitty_at *at, const trt_kitty_shape *s)
{
    const int payload = 4 * trt_kitty_chunk_pixels(s, at->chunk);
    if (at->chunk >= s->chunks)
        return TRT_KITTY_BEHIND;
    if (at->r < 0)
        return at->r < -TRT_KITTY_HEADER_BYTES ? TRT_KITTY_IN_HOME : at->chunk == 0 ? TRT_KITTY_IN_HEADER : TRT_KITTY_IN_CHUNK_HEADER;
    return at->r < payload ? TRT_KITTY_IN_PAYLOAD : at->r < payload + TRT_KITTY_END ? TRT_KITTY_IN_END : TRT_KITTY_BEHIND;
}

/* the pixel of a payload position */
TRT_KITTY_HD int trt_kitty_pixel(const trt_kitty_at *at) { return TRT_KITTY_CHUNK_PIXELS * at->chunk + (at->r >> 2); }

/* the one 64-bit division, by a constant */
TRT_KITTY_HD trt_kitty_at trt_kitty_locate(unsigned long long position)
{
    const unsigned long long front = TRT_KITTY_FIRST - TRT_KITTY_CHUNK_HEADER_BYTES; /* 46: where chunk 1's header would begin, were chunk 0 a stride in front */
    trt_kitty_at at = {0, (int)position - TRT_KITTY_FIRST};
    if (position >= front)
    {
        const unsigned long long chunk = (position - front) / TRT_KITTY_STRIDE;
        at.chunk = (int)chunk;
        at.r = (int)(position - front - chunk * TRT_KITTY_STRIDE) - TRT_KITTY_CHUNK_HEADER_BYTES;
    }
    return at;
}

/* the position d < 4106 bytes behind *from */
TRT_KITTY_HD trt_kitty_at trt_kitty_advance(const trt_kitty_at *from, unsigned d)
{
    const int r = from->r + (int)d, next = r >= TRT_KITTY_PAYLOAD + TRT_KITTY_END;
    const trt_kitty_at at = {from->chunk + next, next ? r - TRT_KITTY_STRIDE : r};
    return at;
}

/* the first pixel at or behind a position (P or more: none) and the last one at or in front of it (-1: none) */
TRT_KITTY_HD int trt_kitty_pixel_from(const trt_kitty_at *at, const trt_kitty_shape *s)
{
    if (at->chunk >= s->chunks)
        return s->pixels;
    if (at->r < 0)
        return TRT_KITTY_CHUNK_PIXELS * at->chunk;
    return at->r < 4 * trt_kitty_chunk_pixels(s, at->chunk) ? trt_kitty_pixel(at) : TRT_KITTY_CHUNK_PIXELS * (at->chunk + 1);
}

TRT_KITTY_HD int trt_kitty_pixel_upto(const trt_kitty_at *at, const trt_kitty_shape *s)
{
    const int n = trt_kitty_chunk_pixels(s, at->chunk);
    if (at->chunk >= s->chunks)
        return s->pixels - 1;
    if (at->r < 0)
        return TRT_KITTY_CHUNK_PIXELS * at->chunk - 1;
    return at->r < 4 * n ? trt_kitty_pixel(at) : TRT_KITTY_CHUNK_PIXELS * at->chunk + n - 1;
}

/* ---- what stands there ---- */

#define TRT_KITTY_PACK8_OF(text, at)                                                                                                            \
    TRT_TEXT_PACK8((unsigned char)(text)[(at)], (unsigned char)(text)[(at) + 1], (unsigned char)(text)[(at) + 2], (unsigned char)(text)[(at) + 3], \
                   (unsigned char)(text)[(at) + 4], (unsigned char)(text)[(at) + 5], (unsigned char)(text)[(at) + 6], (unsigned char)(text)[(at) + 7])

/* digit `place` (0: the ten thousands .. 4: the units) of value <= 99999 */
TRT_KITTY_HD unsigned trt_kitty_digit(unsigned value, int place)
{
    const unsigned q = place == 0 ? value / 10000u : place == 1 ? value / 1000u : place == 2 ? value / 100u : place == 3 ? value / 10u : value;
    return q % 10u;
}

/* byte i < 48 of the first header: the literal, selected by position, and its digits */
TRT_KITTY_HD unsigned trt_kitty_header_byte(int i, int width, int rows, unsigned more)
{
    const unsigned long long k0 = TRT_KITTY_PACK8_OF(TRT_KITTY_HEADER, 0), k1 = TRT_KITTY_PACK8_OF(TRT_KITTY_HEADER, 8), k2 = TRT_KITTY_PACK8_OF(TRT_KITTY_HEADER, 16),
                             k3 = TRT_KITTY_PACK8_OF(TRT_KITTY_HEADER, 24), k4 = TRT_KITTY_PACK8_OF(TRT_KITTY_HEADER, 32), k5 = TRT_KITTY_PACK8_OF(TRT_KITTY_HEADER, 40);
    const unsigned long long k = i < 8 ? k0 : i < 16 ? k1 : i < 24 ? k2 : i < 32 ? k3 : i < 40 ? k4 : k5;
    const unsigned in_width = (unsigned)(i - TRT_KITTY_WIDTH_AT) < 5u, in_rows = (unsigned)(i - TRT_KITTY_ROWS_AT) < 5u;
    const unsigned digit = in_width | in_rows ? trt_kitty_digit((unsigned)(in_width ? width : rows), i - (in_width ? TRT_KITTY_WIDTH_AT : TRT_KITTY_ROWS_AT))
                                              : i == TRT_KITTY_MORE_AT ? more : 0u;
    return ((unsigned)(k >> ((i & 7) * 8)) & 0xffu) + digit;
}

/* what stands at *at inside the text; `chars`: the four characters of the pixel of a payload position */
TRT_KITTY_HD unsigned trt_kitty_byte(const trt_kitty_at *at, const trt_kitty_shape *s, int width, int rows, unsigned chars)
{
    const unsigned long long home = TRT_TEXT_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0), chunk_header = TRT_KITTY_PACK8_OF(TRT_KITTY_CHUNK_HEADER, 0);
    const unsigned more = (unsigned)(at->chunk < s->chunks - 1);
    switch (trt_kitty_what(at, s))
    {
    case TRT_KITTY_IN_HOME:
        return (unsigned)(home >> ((at->r + TRT_KITTY_FIRST) * 8)) & 0xffu;
    case TRT_KITTY_IN_HEADER:
        return trt_kitty_header_byte(at->r + TRT_KITTY_HEADER_BYTES, width, rows, more);
    case TRT_KITTY_IN_CHUNK_HEADER:
        return ((unsigned)(chunk_header >> ((at->r + TRT_KITTY_CHUNK_HEADER_BYTES) * 8)) & 0xffu) + (at->r + TRT_KITTY_CHUNK_HEADER_BYTES == TRT_KITTY_CHUNK_MORE_AT ? more : 0u);
    case TRT_KITTY_IN_PAYLOAD:
        return (chars >> ((at->r & 3) * 8)) & 0xffu;
    case TRT_KITTY_IN_END:
        return at->r & 1 ? '\\' : 0x1bu; /* a payload is a multiple of four bytes: the terminator's first byte stands at an even r */
    default:
        return 0u;
    }
}

/* The pixels the word of four bytes from *at shows: *first the pixel of its first payload byte, *last that of its last one -- the same
 * or its neighbour, of one chunk -- both -1 when it shows none.  1 when all four bytes are payload. */
TRT_KITTY_HD int trt_kitty_word_pixels(const trt_kitty_at *at, const trt_kitty_shape *s, int *first, int *last)
{
    int whole = 1;
    *first = *last = -1;
    for (unsigned b = 0; b < 4; b++)
    {
        const trt_kitty_at here = trt_kitty_advance(at, b);
        const int in = trt_kitty_what(&here, s) == TRT_KITTY_IN_PAYLOAD, p = trt_kitty_pixel(&here);
        *first = in && *first < 0 ? p : *first;
        *last = in ? p : *last;
        whole &= in;
    }
    return whole;
}

/* the word of four bytes from *at, the first in the low byte; chars_first and chars_last: the characters of trt_kitty_word_pixels' two.
 * Bytes behind the text are 0 (the tail's word). */
TRT_KITTY_HD unsigned trt_kitty_word(const trt_kitty_at *at, const trt_kitty_shape *s, int width, int rows, int whole, int first, unsigned chars_first,
                                     unsigned chars_last)
{
    if (whole) /* a byte align of the two registers */
        return (unsigned)(((unsigned long long)chars_last << 32 | chars_first) >> ((at->r & 3) * 8));
    unsigned word = 0;
    for (unsigned b = 0; b < 4; b++)
    {
        const trt_kitty_at here = trt_kitty_advance(at, b);
        word |= trt_kitty_byte(&here, s, width, rows, trt_kitty_pixel(&here) == first ? chars_first : chars_last) << (8 * b);
    }
    return word;
}

/* ---- who stores what ---- */

/* word slots of a text: its words, and one for the tail */
TRT_KITTY_HD unsigned long long trt_kitty_slots(const trt_text_split *split) { return split->words + (split->tail != 0); }

/* waves of ONE text at `address`, and the most any alignment needs (the frames of a batch start anywhere) */
TRT_KITTY_HD unsigned long long trt_kitty_waves(unsigned long long address, unsigned long long bytes)
{
    const trt_text_split split = trt_text_split_of(address, bytes);
    return trt_text_waves(trt_kitty_kind(), trt_kitty_slots(&split));
}
TRT_KITTY_HD unsigned long long trt_kitty_waves_most(unsigned long long bytes) { return trt_text_waves(trt_kitty_kind(), (bytes + 3) / 4); }

typedef struct
{
    trt_kitty_at from; /* the wave's first byte */
    int p0;            /* the first pixel at or behind it: lane l forms p0 + l */
    int count;         /* pixels the wave's bytes show, <= 65: lanes l < min(count, 64) form one, lane 63 forms p0 + 64 too when count is 65 */
} trt_kitty_wave;

/* wave `wave` of a text whose split is *split; 0 when it has no slot (count is then 0 too) */
TRT_KITTY_HD int trt_kitty_wave_of(const trt_text_split *split, const trt_kitty_shape *s, unsigned long long wave, trt_kitty_wave *w)
{
    const unsigned long long first = trt_text_lane_word(trt_kitty_kind(), wave, 0, 0), slots = trt_kitty_slots(split);
    w->p0 = w->count = 0;
    if (first >= slots)
        return 0;
    /* its bytes: whole words, and the tail's bytes where the last slot is the tail's */
    const unsigned long long end = first + TRT_KITTY_WAVE_WORDS <= split->words ? 4 * (first + TRT_KITTY_WAVE_WORDS) : 4 * split->words + split->tail;
    w->from = trt_kitty_locate(split->head + 4 * first);
    const trt_kitty_at last = trt_kitty_advance(&w->from, (unsigned)(end - 4 * first) - 1u);
    w->p0 = trt_kitty_pixel_from(&w->from, s);
    w->count = trt_kitty_pixel_upto(&last, s) - w->p0 + 1;
    if (w->count < 0)
        w->count = 0;
    return 1;
}

#endif /* TRT_KITTY_H */
