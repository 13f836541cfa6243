/* ansi_half_check.c -- csrc/trt_ansi_half.h, the layout of a frame's half-block terminal text and the lane map of the device pass that writes it,
 * compiled for the host and held against the sequential emitter trt_emitter_half_rgb8 (csrc/host/trt_emit.c).  A program of its own:
 * tests/test_ansi_half_layout.py builds and runs it plain and under -fsanitize=address,undefined.
 *
 * For every width 1..70 x rows 1..5 and for 160 x 48, 480 x 280 and 1920 x 1080:
 *  (1) layout: the text assembled position by position through trt_ansi_half_locate / trt_ansi_half_byte equals the emitter's; every position is
 *      classified exactly once (6 prefix bytes, every byte of every cell, 5 end bytes per text row); trt_ansi_half_text_bytes equals the emitter's
 *      length; trt_ansi_half_advance from a located position, and trt_ansi_half_step, agree with trt_ansi_half_locate at every byte.
 *  (2) lane map: a model of the wave of csrc/trt_ansi_half.hpp -- the same header functions in the same order, two arrays for the wave's registers
 *      and an index for the cross-lane read -- for batches of 1..3 frames at every residue of the output address modulo the 4-byte store: every
 *      byte of every frame is stored exactly once, with the emitter's value, and nothing outside is stored; the cells of every wave's span number
 *      at most 64 (TRT_ANSI_HALF_SPAN_CELLS, the header's bound); the head lies in the prefix and the tail in the last 5 bytes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_half.h"
#include "trt_host.h"

#if TRT_ANSI_HALF_SPAN_CELLS > 64 || TRT_ANSI_HALF_WAVE_WORDS % 64 != 0
#error "a wave's cells must fit its 64 lanes, and its words its lanes' turns"
#endif

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_byte(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 56);
}

static int g_failures;
#define FAIL(...)                                             \
    do                                                        \
    {                                                         \
        if (g_failures++ < 20)                                \
        {                                                     \
            fprintf(stderr, "ansi_half_check: " __VA_ARGS__); \
            fputc('\n', stderr);                              \
        }                                                     \
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

/* the two pixels of the cell (trow, col): what a lane of the device pass forms; the lower one of an odd frame's last row is 0 and is not read */
static void cell_pixels(const unsigned char *rgb, int width, int rows, long long trow, int col, unsigned *upper, unsigned *lower)
{
    *upper = *lower = 0u;
    if (2 * trow < rows)
    {
        const long long p = 2 * trow * width + col;
        *upper = packed(rgb, p);
        if (2 * trow + 1 < rows)
            *lower = packed(rgb, p + width);
    }
}

static char *emitter_text(int width, int rows, const unsigned char *rgb, size_t *size)
{
    const size_t room = (size_t)trt_ansi_half_text_bytes(width, rows);
    char *text = (char *)malloc(room);
    if (!text || trt_emitter_half_rgb8(rgb, width, rows, text, room, size) != TRT_HOST_OK)
    {
        fprintf(stderr, "ansi_half_check: no emitter text for %d x %d\n", width, rows);
        exit(2);
    }
    return text;
}

static int same_at(const trt_ansi_half_at *a, const trt_ansi_half_at *b, long long trows)
{
    if (a->r < 0 || b->r < 0)
        return a->r == b->r && a->trow == b->trow;
    if (a->trow >= trows || b->trow >= trows)
        return a->trow == b->trow;
    return a->trow == b->trow && a->r == b->r && a->col == b->col && a->c == b->c;
}

static void check_layout(int width, int rows, int all_starts)
{
    const long long pixels = (long long)width * rows, trows = trt_ansi_half_text_rows(rows), cells_n = trows * width;
    unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3);
    fill_rgb(rgb, pixels);
    size_t size;
    char *want = emitter_text(width, rows, rgb, &size);
    const unsigned long long bytes = trt_ansi_half_text_bytes(width, rows);
    if (bytes != size || bytes != 6ull + (39ull * (unsigned)width + 5) * (unsigned long long)((rows + 1) / 2))
        FAIL("%d x %d: trt_ansi_half_text_bytes %llu, the emitter wrote %zu", width, rows, bytes, size);
    unsigned char *cells = (unsigned char *)calloc((size_t)cells_n, TRT_ANSI_HALF_CELL);
    long long prefix = 0, ends = 0;
    for (unsigned long long t = 0; t < bytes && t < size; t++)
    {
        const trt_ansi_half_at at = trt_ansi_half_locate(t, width, rows);
        const long long cell = trt_ansi_half_cell(&at, width);
        unsigned upper = 0xABCDEFu, lower = 0x123456u;
        if (at.r < 0)
            prefix += at.r == (long long)t - TRT_ANSI_HALF_HOME;
        else if (at.trow >= trows)
            FAIL("%d x %d: position %llu located behind the text", width, rows, t);
        else if (at.c >= TRT_ANSI_HALF_CELL)
            ends += at.col == width - 1 && at.c < TRT_ANSI_HALF_CELL + TRT_ANSI_HALF_END && at.trow == ends / TRT_ANSI_HALF_END &&
                    at.c - TRT_ANSI_HALF_CELL == ends % TRT_ANSI_HALF_END;
        else if (cell < 0 || cell >= cells_n || at.c < 0 || at.col < 0 || at.col >= width || cells[cell * TRT_ANSI_HALF_CELL + at.c]++)
            FAIL("%d x %d: position %llu classified as byte %d of cell %lld once more or out of range", width, rows, t, at.c, cell);
        if (at.r >= 0 && at.trow < trows)
            cell_pixels(rgb, width, rows, at.trow, at.col, &upper, &lower);
        const unsigned got = trt_ansi_half_byte(&at, upper, lower);
        if (got != (unsigned char)want[t])
            FAIL("%d x %d: position %llu is 0x%02x, the emitter has 0x%02x", width, rows, t, got, (unsigned char)want[t]);
    }
    if (prefix != TRT_ANSI_HALF_HOME || ends != TRT_ANSI_HALF_END * trows)
        FAIL("%d x %d: %lld prefix bytes, %lld end bytes", width, rows, prefix, ends);
    for (long long i = 0; i < cells_n * TRT_ANSI_HALF_CELL; i++)
        if (cells[i] != 1)
        {
            FAIL("%d x %d: byte %lld of cell %lld classified %d times", width, rows, i % TRT_ANSI_HALF_CELL, i / TRT_ANSI_HALF_CELL, cells[i]);
            break;
        }
    /* the 32-bit walk against the division, from the starts a wave can have: head + 4 * TRT_ANSI_HALF_WAVE_WORDS * g -- and, for small screens,
     * from every position -- at every byte of the span; and the cells a span touches */
    const unsigned magic = trt_ansi_half_row_magic(width);
    for (unsigned long long start = 0; start < bytes; start += all_starts ? 1 : TRT_ANSI_HALF_SPAN)
        for (unsigned head = 0; head < (all_starts ? 1u : 4u); head++)
        {
            const trt_ansi_half_at from = trt_ansi_half_locate(start + head, width, rows);
            trt_ansi_half_at walk = from;
            const long long c0 = trt_ansi_half_cell(&from, width);
            for (unsigned d = 0; d < TRT_ANSI_HALF_SPAN && start + head + d < bytes; d++)
            {
                const trt_ansi_half_at direct = trt_ansi_half_locate(start + head + d, width, rows),
                                       jumped = trt_ansi_half_advance(&from, d, width, rows, magic);
                if (!same_at(&direct, &jumped, trows) || !same_at(&direct, &walk, trows))
                {
                    FAIL("%d x %d: %u bytes behind position %llu: located row %lld r %lld col %d c %d, advanced row %lld r %lld col %d c %d, walked row %lld r %lld col %d c %d",
                         width, rows, d, start + head, direct.trow, direct.r, direct.col, direct.c, jumped.trow, jumped.r, jumped.col, jumped.c, walk.trow,
                         walk.r, walk.col, walk.c);
                    break;
                }
                const long long rel = trt_ansi_half_cell(&direct, width) - c0;
                if (rel < 0 || rel >= TRT_ANSI_HALF_SPAN_CELLS)
                {
                    FAIL("%d x %d: %u bytes behind position %llu stands cell %lld of the span, the bound is %d", width, rows, d, start + head, rel, TRT_ANSI_HALF_SPAN_CELLS);
                    break;
                }
                const long long before = trt_ansi_half_cell(&walk, width);
                const int moved = trt_ansi_half_step(&walk, width, rows);
                if (start + head + d + 1 < bytes && moved != (trt_ansi_half_cell(&walk, width) != before))
                    FAIL("%d x %d: the step behind position %llu reports %d", width, rows, start + head + d, moved);
            }
        }
    free(cells);
    free(want);
    free(rgb);
}

/* the wave of csrc/trt_ansi_half.hpp: `upper` and `lower` are its 2 x 64 registers, stores are counted */
static void model_wave(unsigned char *memory, unsigned char *count, size_t out, int width, int rows, unsigned row_magic, unsigned width_magic, unsigned long long wave,
                       const unsigned char *rgb)
{
    const unsigned long long bytes = trt_ansi_half_text_bytes(width, rows);
    const trt_ansi_half_split split = trt_ansi_half_split_of((unsigned long long)out, bytes);
    if (split.head > 3 || split.tail > 3 || split.head > TRT_ANSI_HALF_HOME || split.head + 4 * split.words < bytes - TRT_ANSI_HALF_END ||
        split.head + 4 * split.words + split.tail != bytes)
        FAIL("%d x %d at %zu: head %u, %llu words, tail %u of %llu bytes", width, rows, out, split.head, split.words, split.tail, bytes);
    for (int lane = 0; lane < 64 && wave == 0; lane++)
    {
        const long long lone = trt_ansi_half_lone_byte(&split, lane);
        if (lone >= 0)
        {
            if (!(lone < TRT_ANSI_HALF_HOME || lone >= (long long)bytes - TRT_ANSI_HALF_END))
                FAIL("%d x %d: the lone byte %lld lies neither in the prefix nor in the last 5 bytes", width, rows, lone);
            memory[out + lone] = (unsigned char)trt_ansi_half_lone_value(lone, bytes), count[out + lone]++;
        }
    }
    const unsigned long long first = trt_ansi_half_lane_word(wave, 0, 0);
    if (first >= split.words)
        return;
    const trt_ansi_half_at from = trt_ansi_half_locate(split.head + 4 * first, width, rows);
    const long long c0 = trt_ansi_half_cell(&from, width);
    unsigned upper[64], lower[64];
    for (int lane = 0; lane < 64; lane++)
    {
        long long trow;
        int col;
        trt_ansi_half_lane_cell(&from, lane, width, width_magic, &trow, &col);
        if (trow * width + col != c0 + lane || col < 0 || col >= width)
            FAIL("%d x %d: lane %d of wave %llu holds row %lld col %d, its cell is %lld", width, rows, lane, wave, trow, col, c0 + lane);
        cell_pixels(rgb, width, rows, trow, col, &upper[lane], &lower[lane]);
    }
    for (int j = 0; j < TRT_ANSI_HALF_WAVE_WORDS / 64; j++)
        for (int lane = 0; lane < 64; lane++)
        {
            const unsigned long long k = trt_ansi_half_lane_word(wave, lane, j);
            trt_ansi_half_at at = trt_ansi_half_advance(&from, 4u * (unsigned)(64 * j + lane), width, rows, row_magic);
            const long long rel = trt_ansi_half_cell(&at, width) - c0;
            if (k < split.words && (rel < 0 || rel > 63))
                FAIL("%d x %d: word %llu reads the cell %lld behind its wave's first", width, rows, k, rel);
            const unsigned up = upper[(int)rel & 63], lo = lower[(int)rel & 63];
            unsigned word = trt_ansi_half_byte(&at, up, lo);
            for (int b = 1; b < 4; b++)
            {
                (void)trt_ansi_half_step(&at, width, rows);
                word |= trt_ansi_half_byte(&at, up, lo) << (8 * b);
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
    const unsigned long long bytes = trt_ansi_half_text_bytes(width, rows);
    const unsigned row_magic = trt_ansi_half_row_magic(width), width_magic = trt_ansi_half_width_magic(width);
    enum { GUARD = 64 };
    if (bytes < 50)
        FAIL("%d x %d: a text of %llu bytes", width, rows, bytes);
    for (int frames = 1; frames <= 3; frames++)
        for (size_t offset = 0; offset < 4; offset++)
        {
            const size_t total = GUARD + 4 + (size_t)bytes * frames + GUARD;
            unsigned char *memory = (unsigned char *)malloc(total), *count = (unsigned char *)calloc(total, 1);
            unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3 * frames);
            memset(memory, 0xA5, total); /* offsets stand for addresses: the block's own address plays no part */
            fill_rgb(rgb, pixels * frames);
            /* a batch's grid: the most waves any alignment needs; a single frame's: those of its own alignment */
            const unsigned long long waves = frames > 1 ? trt_ansi_half_waves(bytes / 4) : trt_ansi_half_waves(trt_ansi_half_split_of(GUARD + offset, bytes).words);
            for (int b = 0; b < frames; b++)
                for (unsigned long long wave = 0; wave < waves; wave++)
                    model_wave(memory, count, GUARD + offset + (size_t)b * bytes, width, rows, row_magic, width_magic, wave, rgb + (size_t)b * pixels * 3);
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
    static const int larger[][2] = {{160, 48}, {480, 280}, {1920, 1080}};
    if (trt_ansi_half_text_bytes(0, 5) || trt_ansi_half_text_bytes(5, 0) || trt_ansi_half_text_bytes(-1, -1) || trt_ansi_half_text_bytes(160, 48) != 149886 ||
        trt_ansi_half_text_bytes(480, 280) != 2621506 || trt_ansi_half_text_bytes(1, 1) != 50)
        FAIL("trt_ansi_half_text_bytes of an empty screen, of 1 x 1, of 160 x 48 or of 480 x 280");
    if ((TRT_ANSI_HALF_CELL - 1 + TRT_ANSI_HALF_SPAN - 1) / TRT_ANSI_HALF_CELL + 1 != TRT_ANSI_HALF_SPAN_CELLS || TRT_ANSI_HALF_SPAN_CELLS > 64)
        FAIL("a span of %d bytes touches up to %d cells", TRT_ANSI_HALF_SPAN, TRT_ANSI_HALF_SPAN_CELLS);
    for (int width = 1; width <= 70; width++)
        for (int rows = 1; rows <= 5; rows++)
        {
            check_layout(width, rows, width <= 6 || width == 58 || width == 59);
            check_lane_map(width, rows);
        }
    for (size_t i = 0; i < sizeof larger / sizeof larger[0]; i++)
    {
        check_layout(larger[i][0], larger[i][1], 0);
        check_lane_map(larger[i][0], larger[i][1]);
    }
    for (int ch = 0; ch < 3; ch++)
        for (int v = 0; v < 256; v++)
            if (!g_seen[ch][v])
                FAIL("channel %d never took the value %d", ch, v);
    if (g_failures)
    {
        fprintf(stderr, "ansi_half_check: %d failure(s)\n", g_failures);
        return 1;
    }
    puts("ansi_half_check: ok");
    return 0;
}
