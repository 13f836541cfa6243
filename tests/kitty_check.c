/* kitty_check.c -- csrc/trt_kitty.h, the format of a frame as a kitty graphics-protocol image with the position map and the lane map of the device
 * pass that writes it, compiled for the host and held against the sequential emitter trt_emitter_kitty_rgb8 (csrc/host/trt_emit.c).  A program of
 * its own: tests/test_kitty_layout.py builds and runs it plain and under -fsanitize=address,undefined.  For every P in 1..70, 1020..1030, 2044..2052
 * and 4095..4098, each as every width x rows with that product, and for 160 x 48, 480 x 280 and 1920 x 1080:
 *
 *  (1) layout: the text assembled position by position through trt_kitty_locate and trt_kitty_byte equals the emitter's; every position is
 *      classified exactly once (6 prefix bytes, 48 header bytes, 8 bytes per later chunk's header, every character of every pixel, 2 terminator
 *      bytes per chunk), positions behind the text as such; trt_kitty_advance agrees with trt_kitty_locate at every byte of a span from every start
 *      a wave can have (from every position where the text is short); the header's length is the emitter's.
 *  (2) lane map: model_wave is kitty_write of csrc/trt_kitty.hpp -- the same functions in the same order -- for batches of 1..3 frames at every
 *      residue of the output address modulo the 4-byte store, in memory with guards either side: every byte of every frame is stored exactly once,
 *      with the emitter's value, and nothing outside; words are stored at aligned addresses; a wave's pixels number at most 65 and a word reads
 *      only lanes that formed one (the 65th from lane 63's second register); no pixel is formed more than twice and a wave forms at most one pixel
 *      that another wave has formed before it.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_kitty.h"
#include "trt_host.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_byte(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 56);
}

static int g_failures;
#define FAIL(...)                                      \
    do                                                 \
    {                                                  \
        if (g_failures++ < 20)                         \
        {                                              \
            fprintf(stderr, "kitty_check: " __VA_ARGS__); \
            fputc('\n', stderr);                       \
        }                                              \
    } while (0)

static unsigned char g_seen[3][256]; /* values every channel has taken over the run */

static void fill_rgb(unsigned char *rgb, long long pixels)
{
    for (long long p = 0; p < pixels; p++)
        for (int ch = 0; ch < 3; ch++)
        {
            const unsigned v = next_byte();
            rgb[3 * p + ch] = (unsigned char)v;
            g_seen[ch][v] = 1;
        }
}

static unsigned packed(const unsigned char *rgb, long long p) { return (unsigned)rgb[3 * p] | (unsigned)rgb[3 * p + 1] << 8 | (unsigned)rgb[3 * p + 2] << 16; }

static char *emitter_text(int width, int rows, const unsigned char *rgb, size_t *size)
{
    const size_t room = (size_t)trt_kitty_text_bytes(width, rows);
    char *text = (char *)malloc(room);
    if (!text || trt_emitter_kitty_rgb8(rgb, width, rows, text, room, size) != TRT_HOST_OK)
    {
        fprintf(stderr, "kitty_check: no emitter text for %d x %d\n", width, rows);
        exit(2);
    }
    return text;
}

static void check_layout(int width, int rows)
{
    const trt_kitty_shape shape = trt_kitty_shape_of(width, rows);
    const long long pixels = (long long)width * rows;
    unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3);
    fill_rgb(rgb, pixels);
    size_t size;
    char *want = emitter_text(width, rows, rgb, &size);
    const unsigned long long bytes = trt_kitty_text_bytes(width, rows);
    if (bytes != size || shape.pixels != pixels || shape.chunks != (pixels + 1023) / 1024 || bytes != 4ull * (unsigned long long)pixels + 10ull * (unsigned long long)shape.chunks + 46)
        FAIL("%d x %d: the header's text has %llu bytes, the emitter's %zu", width, rows, bytes, size);
    unsigned char *chars = (unsigned char *)calloc((size_t)pixels, 4);
    long long home = 0, header = 0, chunk_headers = 0, ends = 0;
    for (unsigned long long t = 0; t < bytes + 8; t++)
    {
        const trt_kitty_at at = trt_kitty_locate(t);
        const int what = trt_kitty_what(&at, &shape);
        if (t >= bytes)
        {
            if (what != TRT_KITTY_BEHIND || trt_kitty_byte(&at, &shape, width, rows, 0xffffffffu) != 0)
                FAIL("%d x %d: position %llu behind the text is classified as %d", width, rows, t, what);
            continue;
        }
        unsigned held = 0xA5A5A5A5u;
        switch (what)
        {
        case TRT_KITTY_IN_HOME:
            home += at.chunk == 0 && at.r + TRT_KITTY_FIRST == (long long)t;
            break;
        case TRT_KITTY_IN_HEADER:
            header += at.chunk == 0 && at.r + TRT_KITTY_HEADER_BYTES == header;
            break;
        case TRT_KITTY_IN_CHUNK_HEADER:
            chunk_headers += at.chunk == 1 + chunk_headers / 8 && at.r + 8 == chunk_headers % 8;
            break;
        case TRT_KITTY_IN_END:
            ends += at.chunk == ends / 2 && at.r - 4 * trt_kitty_chunk_pixels(&shape, at.chunk) == ends % 2;
            break;
        case TRT_KITTY_IN_PAYLOAD:
        {
            const int p = trt_kitty_pixel(&at);
            if (p < 0 || p >= pixels || p / 1024 != at.chunk || chars[4 * (size_t)p + (at.r & 3)]++)
                FAIL("%d x %d: position %llu classified as character %d of pixel %d once more or out of range", width, rows, t, at.r & 3, p);
            else
                held = trt_kitty_chars(packed(rgb, p));
            break;
        }
        default:
            FAIL("%d x %d: position %llu inside the text is classified as behind it", width, rows, t);
        }
        const unsigned got = trt_kitty_byte(&at, &shape, width, rows, held);
        if (got != (unsigned char)want[t])
            FAIL("%d x %d: position %llu is 0x%02x, the emitter has 0x%02x", width, rows, t, got, (unsigned char)want[t]);
    }
    if (home != TRT_KITTY_HOME || header != TRT_KITTY_HEADER_BYTES || chunk_headers != 8ll * (shape.chunks - 1) || ends != 2ll * shape.chunks)
        FAIL("%d x %d: %lld prefix bytes, %lld header bytes, %lld bytes of later headers, %lld terminator bytes", width, rows, home, header, chunk_headers, ends);
    for (long long i = 0; i < 4 * pixels; i++)
        if (chars[i] != 1)
        {
            FAIL("%d x %d: character %lld of pixel %lld classified %d times", width, rows, i % 4, i / 4, chars[i]);
            break;
        }
    /* the compare against the division: from the starts a wave can have -- from every position of a short text -- at every byte of a span and a
     * little behind the text; and the pixels a span shows */
    const int every = bytes < 6000;
    for (unsigned long long start = 0; start < bytes; start += every ? 1 : TRT_KITTY_SPAN)
        for (unsigned head = 0; head < (every ? 1u : 4u); head++)
        {
            const trt_kitty_at from = trt_kitty_locate(start + head);
            int low = -1, high = -1;
            for (unsigned d = 0; d < TRT_KITTY_SPAN + 4 && start + head + d < bytes + 8; d++)
            {
                const trt_kitty_at direct = trt_kitty_locate(start + head + d), jumped = trt_kitty_advance(&from, d);
                const int what = trt_kitty_what(&direct, &shape);
                if (what != trt_kitty_what(&jumped, &shape) || (what != TRT_KITTY_BEHIND && (direct.chunk != jumped.chunk || direct.r != jumped.r)))
                {
                    FAIL("%d x %d: %u bytes behind position %llu: located chunk %d r %d, advanced chunk %d r %d", width, rows, d, start + head, direct.chunk, direct.r,
                         jumped.chunk, jumped.r);
                    break;
                }
                if (d < TRT_KITTY_SPAN && what == TRT_KITTY_IN_PAYLOAD)
                {
                    high = trt_kitty_pixel(&direct);
                    low = low < 0 ? high : low;
                    if (trt_kitty_pixel_from(&direct, &shape) != high || trt_kitty_pixel_upto(&direct, &shape) != high)
                        FAIL("%d x %d: the pixel at or behind, or at or in front of, position %llu", width, rows, start + head + d);
                }
            }
            if (low >= 0 && (trt_kitty_pixel_from(&from, &shape) != low || high - low + 1 > TRT_KITTY_SPAN_PIXELS))
                FAIL("%d x %d: the span from position %llu shows the pixels %d .. %d, the first at or behind it is %d", width, rows, start + head, low, high,
                     trt_kitty_pixel_from(&from, &shape));
        }
    free(chars);
    free(want);
    free(rgb);
}

/* kitty_write of csrc/trt_kitty.hpp for the 64 lanes of a wave: `mine` and `extra` are its registers; stores and formed pixels are counted.
 * Returns the pixels this wave formed that were formed before. */
static int model_wave(unsigned char *memory, unsigned char *count, size_t out, int width, int rows, unsigned long long wave, const unsigned char *rgb,
                      unsigned char *formed)
{
    const trt_kitty_shape shape = trt_kitty_shape_of(width, rows);
    const unsigned long long bytes = trt_kitty_text_bytes(width, rows);
    const trt_text_split split = trt_text_split_of((unsigned long long)out, bytes);
    int again = 0;
    if (split.head > 3 || split.tail > 3 || split.head > TRT_KITTY_HOME || split.head + 4 * split.words + split.tail != bytes)
        FAIL("%d x %d at %zu: head %u, %llu words, tail %u of %llu bytes", width, rows, out, split.head, split.words, split.tail, bytes);
    for (int lane = 0; lane < 64 && wave == 0; lane++)
        if (lane < (int)split.head)
        {
            const trt_kitty_at at = trt_kitty_locate((unsigned long long)lane);
            memory[out + lane] = (unsigned char)trt_kitty_byte(&at, &shape, width, rows, 0u), count[out + lane]++;
        }
    trt_kitty_wave w;
    if (!trt_kitty_wave_of(&split, &shape, wave, &w))
    {
        if (w.count)
            FAIL("%d x %d: wave %llu has no slot and %d pixels", width, rows, wave, w.count);
        return 0;
    }
    if (w.count < 0 || w.count > TRT_KITTY_SPAN_PIXELS || (w.count && (w.p0 < 0 || w.p0 + w.count > shape.pixels)))
        FAIL("%d x %d: wave %llu shows %d pixels from %d of %d", width, rows, wave, w.count, w.p0, shape.pixels);
    unsigned mine[64], extra = 0u;
    for (int lane = 0; lane < 64; lane++)
    {
        mine[lane] = 0xDEADBEEFu; /* what no lane formed must not show */
        if (lane < w.count)
            mine[lane] = trt_kitty_chars(packed(rgb, w.p0 + lane)), again += formed[w.p0 + lane]++ != 0;
        if (w.count == TRT_KITTY_SPAN_PIXELS && lane == 63)
            extra = trt_kitty_chars(packed(rgb, w.p0 + 64)), again += formed[w.p0 + 64]++ != 0;
    }
    for (int lane = 0; lane < 64; lane++)
    {
        const unsigned long long k = trt_text_lane_word(trt_kitty_kind(), wave, lane, 0);
        const trt_kitty_at at = trt_kitty_advance(&w.from, 4u * (unsigned)lane);
        int first, last;
        const int whole = trt_kitty_word_pixels(&at, &shape, &first, &last);
        const int rel_first = first - w.p0, rel_last = last - w.p0;
        if (k <= split.words && first >= 0 && (rel_first < 0 || rel_last >= w.count || rel_last - rel_first > 1 || first / 1024 != last / 1024))
            FAIL("%d x %d: word %llu shows the pixels %d and %d behind its wave's first of %d", width, rows, k, rel_first, rel_last, w.count);
        const unsigned held_first = mine[rel_first & 63], held_last = mine[rel_last & 63];
        const unsigned word = trt_kitty_word(&at, &shape, width, rows, whole, first, rel_first == 64 ? extra : held_first, rel_last == 64 ? extra : held_last);
        const size_t where = out + split.head + 4 * k;
        if (k < split.words)
        {
            if (where % 4)
                FAIL("%d x %d: word %llu is stored at an address that is %zu modulo 4", width, rows, k, where % 4);
            for (int b = 0; b < 4; b++)
                memory[where + b] = (unsigned char)(word >> (8 * b)), count[where + b]++;
        }
        else if (k == split.words)
            for (unsigned b = 0; b < split.tail; b++)
                memory[where + b] = (unsigned char)(word >> (8 * b)), count[where + b]++;
    }
    return again;
}

static void check_lane_map(int width, int rows)
{
    const long long pixels = (long long)width * rows;
    const unsigned long long bytes = trt_kitty_text_bytes(width, rows);
    enum { GUARD = 64 };
    for (int frames = 1; frames <= 3; frames++)
        for (size_t offset = 0; offset < 4; offset++)
        {
            const size_t total = GUARD + 4 + (size_t)bytes * frames + GUARD;
            unsigned char *memory = (unsigned char *)malloc(total), *count = (unsigned char *)calloc(total, 1);
            unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3 * frames), *formed = (unsigned char *)calloc((size_t)pixels * frames, 1);
            memset(memory, 0xA5, total); /* offsets stand for addresses: the block's own address plays no part */
            fill_rgb(rgb, pixels * frames);
            /* a batch's grid: the most waves any alignment needs; a single frame's: those of its own alignment */
            const unsigned long long waves = frames > 1 ? trt_kitty_waves_most(bytes) : trt_kitty_waves(GUARD + offset, bytes);
            for (int b = 0; b < frames; b++)
                for (unsigned long long wave = 0; wave < waves; wave++)
                    if (model_wave(memory, count, GUARD + offset + (size_t)b * bytes, width, rows, wave, rgb + (size_t)b * pixels * 3, formed + (size_t)b * pixels) > 1)
                        FAIL("%d x %d, %d frame(s) at offset %zu: wave %llu forms more than one pixel that was formed before", width, rows, frames, offset, wave);
            for (long long p = 0; p < pixels * frames; p++)
                if (formed[p] < 1 || formed[p] > 2)
                {
                    FAIL("%d x %d, %d frame(s) at offset %zu: pixel %lld is formed %d times", width, rows, frames, offset, p, formed[p]);
                    break;
                }
            for (size_t i = 0; i < total; i++)
            {
                const int inside = i >= GUARD + offset && i < GUARD + offset + (size_t)bytes * frames;
                if (count[i] != inside || (!inside && memory[i] != 0xA5))
                {
                    FAIL("%d x %d, %d frame(s) at offset %zu: byte %lld of the text is stored %d times", width, rows, frames, offset, (long long)i - (long long)(GUARD + offset), count[i]);
                    break;
                }
            }
            for (int b = 0; b < frames; b++)
            {
                size_t size;
                char *want = emitter_text(width, rows, rgb + (size_t)b * pixels * 3, &size);
                const unsigned char *got = memory + GUARD + offset + (size_t)b * bytes;
                if (size != bytes || memcmp(got, want, size))
                {
                    size_t at = 0;
                    while (at < size && got[at] == (unsigned char)want[at])
                        at++;
                    FAIL("%d x %d, frame %d of %d at offset %zu: differs from the emitter's text at byte %zu of %zu", width, rows, b, frames, offset, at, size);
                }
                free(want);
            }
            free(formed);
            free(rgb);
            free(count);
            free(memory);
        }
}

static void check_every_factoring(int pixels)
{
    for (int width = 1; width <= pixels; width++)
        if (pixels % width == 0)
        {
            check_layout(width, pixels / width);
            check_lane_map(width, pixels / width);
        }
}

static void check_constants(void)
{
    static const char header[] = TRT_KITTY_HEADER, chunk_header[] = TRT_KITTY_CHUNK_HEADER;
    static const char alphabet[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    if (sizeof header - 1 != TRT_KITTY_HEADER_BYTES || sizeof chunk_header - 1 != TRT_KITTY_CHUNK_HEADER_BYTES || TRT_KITTY_STRIDE != 4106 || TRT_KITTY_FIRST != 54 ||
        TRT_KITTY_SPAN != 256)
        FAIL("the header literals' lengths, the stride or the first payload's position");
    if (memcmp(header + TRT_KITTY_WIDTH_AT - 2, "s=00000,", 8) || memcmp(header + TRT_KITTY_ROWS_AT - 2, "v=00000,", 8) || memcmp(header + TRT_KITTY_MORE_AT - 2, "m=0;", 4) ||
        memcmp(chunk_header + TRT_KITTY_CHUNK_MORE_AT - 3, "m=00;", 5))
        FAIL("the places of the header's digits");
    for (unsigned v = 0; v < 64; v++)
        if (trt_kitty_base64(v) != (unsigned char)alphabet[v])
            FAIL("the base64 character of %u", v);
    if (trt_kitty_chars(255u | 0u << 8 | 9u << 16) != ((unsigned)'/' | (unsigned)'w' << 8 | (unsigned)'A' << 16 | (unsigned)'J' << 24))
        FAIL("the characters of the pixel (255, 0, 9)");
    if (trt_kitty_text_bytes(0, 5) || trt_kitty_text_bytes(5, 0) || trt_kitty_text_bytes(-1, -1) || trt_kitty_text_bytes(100000, 1) || trt_kitty_text_bytes(1, 100000) ||
        trt_kitty_text_bytes(1, 1) != 60 || trt_kitty_text_bytes(160, 48) != 30846 || trt_kitty_text_bytes(480, 280) != 538966 || trt_kitty_text_bytes(1920, 1080) != 8314696 ||
        trt_kitty_text_bytes(99999, 99999) != 4ull * 9999800001ull + 10ull * 9765430ull + 46)
        FAIL("trt_kitty_text_bytes of an empty screen, above the limits or of a known size");
}

int main(void)
{
    static const int larger[][2] = {{160, 48}, {480, 280}, {1920, 1080}};
    static const int ranges[][2] = {{1, 70}, {1020, 1030}, {2044, 2052}, {4095, 4098}};
    check_constants();
    for (size_t i = 0; i < sizeof ranges / sizeof ranges[0]; i++)
        for (int pixels = ranges[i][0]; pixels <= ranges[i][1]; pixels++)
            check_every_factoring(pixels);
    for (size_t i = 0; i < sizeof larger / sizeof larger[0]; i++)
    {
        check_layout(larger[i][0], larger[i][1]);
        check_lane_map(larger[i][0], larger[i][1]);
    }
    for (int ch = 0; ch < 3; ch++)
        for (int v = 0; v < 256; v++)
            if (!g_seen[ch][v])
                FAIL("channel %d never took the value %d", ch, v);
    if (g_failures)
    {
        fprintf(stderr, "kitty_check: %d failure(s)\n", g_failures);
        return 1;
    }
    puts("kitty_check: ok");
    return 0;
}
