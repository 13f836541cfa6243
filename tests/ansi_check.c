/* ansi_check.c -- csrc/trt_ansi.h, the layout of a frame's terminal text and the lane map of the device pass that writes it, compiled for the
 * host and held against the host emitter (csrc/host/trt_emit.c).  A program of its own: tests/test_ansi_layout.py builds and runs it plain and
 * under -fsanitize=address,undefined.
 *
 *  (1) layout: for every width 1..70 x rows 1..4 and a few larger screens, the text assembled position by position through trt_ansi_locate /
 *      trt_ansi_byte equals the emitter's buffer after trt_emitter_patch_rgb8; every position is classified exactly once (6 prefix bytes, every
 *      byte of every cell, a newline per row, 3 NULs); trt_ansi_text_bytes equals trt_emitter_size; trt_ansi_advance / trt_ansi_step agree with
 *      trt_ansi_locate from every word-aligned start.
 *  (2) lane map: a model of the wave of csrc/trt_ansi.hpp -- the same header functions in the same order, an array for the wave's registers and an
 *      index for the cross-lane read -- for batches of 1..3 frames at every residue of the output address modulo the 4-byte store: every byte of
 *      every frame is stored exactly once, with the emitter's value, and nothing outside is stored.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi.h"
#include "trt_host.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_byte(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 56);
}

static int g_failures;
#define FAIL(...)                                  \
    do                                             \
    {                                              \
        if (g_failures++ < 20)                     \
        {                                          \
            fprintf(stderr, "ansi_check: " __VA_ARGS__); \
            fputc('\n', stderr);                   \
        }                                          \
    } while (0)

static unsigned char g_seen[3][256]; /* values every channel has taken over the run */

/* pixel p of frame `frame`: random, but the first 256 pixels of a screen walk every value through every channel */
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
    trt_emitter *e = NULL;
    if (trt_emitter_create(width, rows, &e) != TRT_HOST_OK || trt_emitter_patch_rgb8(e, rgb) != TRT_HOST_OK)
    {
        fprintf(stderr, "ansi_check: no emitter for %d x %d\n", width, rows);
        exit(2);
    }
    *size = trt_emitter_size(e);
    char *text = (char *)malloc(*size);
    memcpy(text, trt_emitter_buffer(e), *size);
    trt_emitter_destroy(e);
    return text;
}

static int same_at(const trt_ansi_at *a, const trt_ansi_at *b, long long rows)
{
    if (a->r < 0 || b->r < 0)
        return a->r == b->r && a->row == b->row;
    if (a->row >= rows || b->row >= rows)
        return a->row == b->row && a->r == b->r;
    return a->row == b->row && a->r == b->r && a->col == b->col && a->c == b->c;
}

static void check_layout(int width, int rows, int all_starts)
{
    const long long pixels = (long long)width * rows;
    unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3);
    fill_rgb(rgb, pixels);
    size_t size;
    char *want = emitter_text(width, rows, rgb, &size);
    const unsigned long long bytes = trt_ansi_text_bytes(width, rows);
    if (bytes != size)
        FAIL("%d x %d: trt_ansi_text_bytes %llu, trt_emitter_size %zu", width, rows, bytes, size);
    unsigned char *cells = (unsigned char *)calloc((size_t)pixels, TRT_ANSI_CELL);
    long long prefix = 0, newlines = 0, nuls = 0;
    for (unsigned long long t = 0; t < bytes && t < size; t++)
    {
        const trt_ansi_at at = trt_ansi_locate(t, width, rows);
        const long long p = trt_ansi_pixel(&at, width);
        if (at.r < 0)
            prefix += at.r == (long long)t - TRT_ANSI_HOME;
        else if (at.row >= rows)
            nuls += at.r == nuls; /* the NULs in turn */
        else if (at.c == TRT_ANSI_CELL)
            newlines += at.col == width - 1 && at.row == newlines;
        else if (p < 0 || p >= pixels || at.c < 0 || at.c > TRT_ANSI_CELL || cells[p * TRT_ANSI_CELL + at.c]++)
            FAIL("%d x %d: position %llu classified as byte %d of pixel %lld once more or out of range", width, rows, t, at.c, p);
        const unsigned got = trt_ansi_byte(&at, rows, at.r >= 0 && at.row < rows ? packed(rgb, p) : 0xABCDEFu);
        if (got != (unsigned char)want[t])
            FAIL("%d x %d: position %llu is 0x%02x, the emitter has 0x%02x", width, rows, t, got, (unsigned char)want[t]);
    }
    if (prefix != TRT_ANSI_HOME || newlines != rows || nuls != TRT_ANSI_NULS)
        FAIL("%d x %d: %lld prefix bytes, %lld newlines, %lld NULs", width, rows, prefix, newlines, nuls);
    for (long long i = 0; i < pixels * TRT_ANSI_CELL; i++)
        if (cells[i] != 1)
        {
            FAIL("%d x %d: byte %lld of pixel %lld classified %d times", width, rows, i % TRT_ANSI_CELL, i / TRT_ANSI_CELL, cells[i]);
            break;
        }
    /* the 32-bit walk against the division, from the starts a wave can have: head + 4 * TRT_ANSI_WAVE_WORDS * g -- and, for small screens, from
     * every position */
    const unsigned magic = trt_ansi_row_magic(width);
    for (unsigned long long start = 0; start < bytes; start += all_starts ? 1 : TRT_ANSI_SPAN)
        for (unsigned head = 0; head < (all_starts ? 1u : 4u); head++)
        {
            const trt_ansi_at from = trt_ansi_locate(start + head, width, rows);
            trt_ansi_at walk = from;
            for (unsigned d = 0; d < TRT_ANSI_SPAN; d++)
            {
                const trt_ansi_at direct = trt_ansi_locate(start + head + d, width, rows), jumped = trt_ansi_advance(&from, d, width, rows, magic);
                if (start + head + d < bytes + 8 && (!same_at(&direct, &jumped, rows) || !same_at(&direct, &walk, rows)))
                {
                    FAIL("%d x %d: %u bytes behind position %llu: located row %lld r %lld col %d c %d, advanced row %lld r %lld col %d c %d, walked row %lld r %lld col %d c %d",
                         width, rows, d, start + head, direct.row, direct.r, direct.col, direct.c, jumped.row, jumped.r, jumped.col, jumped.c, walk.row, walk.r,
                         walk.col, walk.c);
                    d = TRT_ANSI_SPAN;
                }
                const long long before = trt_ansi_pixel(&walk, width);
                const int moved = trt_ansi_step(&walk, width, rows);
                if (start + head + d + 1 < bytes - TRT_ANSI_NULS && moved != (trt_ansi_pixel(&walk, width) != before))
                    FAIL("%d x %d: the step behind position %llu reports %d", width, rows, start + head + d, moved);
            }
        }
    free(cells);
    free(want);
    free(rgb);
}

/* the wave of csrc/trt_ansi.hpp: `mine` are its 64 registers, stores are counted */
static void model_wave(unsigned char *memory, unsigned char *count, size_t out, int width, int rows, unsigned magic, unsigned long long wave, const unsigned char *rgb)
{
    const trt_ansi_split split = trt_ansi_split_of((unsigned long long)out, trt_ansi_text_bytes(width, rows));
    for (int lane = 0; lane < 64 && wave == 0; lane++)
    {
        const long long lone = trt_ansi_lone_byte(&split, lane);
        if (lone >= 0)
            memory[out + lone] = (unsigned char)trt_ansi_lone_value(lone), count[out + lone]++;
    }
    const unsigned long long first = trt_ansi_lane_word(wave, 0, 0);
    if (first >= split.words)
        return;
    const trt_ansi_at from = trt_ansi_locate(split.head + 4 * first, width, rows);
    const long long pixels = (long long)width * rows, p0 = trt_ansi_pixel(&from, width);
    unsigned mine[64];
    for (int lane = 0; lane < 64; lane++)
        mine[lane] = p0 + lane < pixels ? packed(rgb, p0 + lane) : 0u;
    for (int j = 0; j < TRT_ANSI_WAVE_WORDS / 64; j++)
        for (int lane = 0; lane < 64; lane++)
        {
            const unsigned long long k = trt_ansi_lane_word(wave, lane, j);
            trt_ansi_at at = trt_ansi_advance(&from, 4u * (unsigned)(64 * j + lane), width, rows, magic), walk = at;
            for (int b = 1; b < 4; b++)
                (void)trt_ansi_step(&walk, width, rows);
            const long long rel_a = trt_ansi_pixel(&at, width) - p0, rel_b = trt_ansi_pixel(&walk, width) - p0;
            if (k < split.words && (rel_a < 0 || rel_b > 63) && at.row < rows)
                FAIL("%d x %d: word %llu reads the pixels %lld and %lld behind its wave's first", width, rows, k, rel_a, rel_b);
            const unsigned rgb_a = mine[(int)rel_a & 63], rgb_b = mine[(int)rel_b & 63];
            unsigned word = trt_ansi_byte(&at, rows, rgb_a), other = 0;
            for (int b = 1; b < 4; b++)
            {
                other |= (unsigned)trt_ansi_step(&at, width, rows);
                word |= trt_ansi_byte(&at, rows, other ? rgb_b : rgb_a) << (8 * b);
            }
            if (k < split.words)
            {
                const size_t where = out + split.head + 4 * k;
                if (where % 4)
                    FAIL("%d x %d: word %llu is stored at an address that is %zu modulo 4", width, rows, k, where % 4);
                for (int b = 0; b < 4; b++)
                    memory[where + b] = (unsigned char)(word >> (8 * b)), count[where + b]++;
            }
        }
}

static void check_lane_map(int width, int rows)
{
    const long long pixels = (long long)width * rows;
    const unsigned long long bytes = trt_ansi_text_bytes(width, rows);
    const unsigned magic = trt_ansi_row_magic(width);
    enum { GUARD = 64 };
    for (int frames = 1; frames <= 3; frames++)
        for (size_t offset = 0; offset < 4; offset++)
        {
            const size_t total = GUARD + 4 + (size_t)bytes * frames + GUARD;
            unsigned char *memory = (unsigned char *)malloc(total), *count = (unsigned char *)calloc(total, 1);
            unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3 * frames);
            memset(memory, 0xA5, total); /* offsets stand for addresses: the block's own address plays no part */
            fill_rgb(rgb, pixels * frames);
            /* a batch's grid: the most waves any alignment needs; a single frame's: those of its own alignment */
            const unsigned long long waves = frames > 1 ? trt_ansi_waves(bytes / 4) : trt_ansi_waves(trt_ansi_split_of(GUARD + offset, bytes).words);
            for (int b = 0; b < frames; b++)
                for (unsigned long long wave = 0; wave < waves; wave++)
                    model_wave(memory, count, GUARD + offset + (size_t)b * bytes, width, rows, magic, wave, rgb + (size_t)b * pixels * 3);
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
                    FAIL("%d x %d, frame %d of %d at offset %zu: differs from the emitter's text at byte %zu", width, rows, b, frames, offset, at);
                }
                free(want);
            }
            free(rgb);
            free(count);
            free(memory);
        }
}

int main(void)
{
    static const int larger[][2] = {{160, 48}, {96, 32}, {333, 7}, {1, 100}, {480, 9}, {1000, 3}};
    static const int mapped[][2] = {{1, 1}, {1, 5}, {2, 3}, {3, 2}, {4, 3}, {7, 5}, {33, 3}, {61, 4}, {62, 3}, {63, 2}, {64, 1}, {65, 2}, {67, 13}, {1, 130}, {2, 70}, {160, 48}, {480, 9}};
    if (trt_ansi_text_bytes(0, 5) || trt_ansi_text_bytes(5, 0) || trt_ansi_text_bytes(-1, -1) || trt_ansi_text_bytes(160, 48) != 192057)
        FAIL("trt_ansi_text_bytes of an empty screen, or of 160 x 48");
    for (int width = 1; width <= 70; width++)
        for (int rows = 1; rows <= 4; rows++)
            check_layout(width, rows, width <= 6 || width == 61 || width == 62);
    for (size_t i = 0; i < sizeof larger / sizeof larger[0]; i++)
        check_layout(larger[i][0], larger[i][1], 0);
    for (size_t i = 0; i < sizeof mapped / sizeof mapped[0]; i++)
        check_lane_map(mapped[i][0], mapped[i][1]);
    for (int ch = 0; ch < 3; ch++)
        for (int v = 0; v < 256; v++)
            if (!g_seen[ch][v])
                FAIL("channel %d never took the value %d", ch, v);
    if (g_failures)
    {
        fprintf(stderr, "ansi_check: %d failure(s)\n", g_failures);
        return 1;
    }
    puts("ansi_check: ok");
    return 0;
}
