/* sixel_check.c -- csrc/trt_sixel.h, the format of a frame as a DEC sixel image with the position map and the lane map of the device kernels
 * that write it, compiled for the host and held against the sequential emitter trt_emitter_sixel_rgb8 (csrc/host/trt_emit.c).  A program of its
 * own: tests/test_sixel_layout.py builds and runs it plain and under -fsanitize=address,undefined.  For the widths 1..9, 63..65, 255..258 and
 * 1025 with the rows 1, 5, 6, 7, 13, for 40 x 6 with every palette colour once, 160 x 48 and 1 x 6151, each with pictures of few colours, of
 * one colour, of every colour and with bands that alternate between 1 and many colours, and at each of the four store alignments:
 *
 *  the text is assembled as the kernels of csrc/trt_sixel.hpp go about it -- the same functions in the same order: the bands' masks and counts
 *  (measure), their exclusive scan, the length, the prologue and the terminator (offsets), then band by band and slot by slot, i.e. thread by
 *  thread, the lane's indices formed once and the walk over the band's mask in ascending order, an aligned word or the bytes of a partial
 *  slot per colour (write) -- into memory with guards either side.  Every byte below the length is stored exactly once and none outside; words
 *  are stored at 4-aligned addresses only; the length and the text are the emitter's; the capacity holds the text.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_sixel.h"
#include "trt_host.h"

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_byte(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 56);
}

static int g_failures;
#define FAIL(...)                                         \
    do                                                    \
    {                                                     \
        if (g_failures++ < 20)                            \
        {                                                 \
            fprintf(stderr, "sixel_check: " __VA_ARGS__); \
            fputc('\n', stderr);                          \
        }                                                 \
    } while (0)

enum
{
    GUARD = 64,
    FEW,       /* a dozen colours, at random */
    ONE,       /* one colour */
    EVERY,     /* pixel p has palette entry 16 + p mod 240 */
    ALTERNATE, /* even bands one colour, odd bands every colour they have room for */
    RANDOM,    /* every byte at random */
    KINDS_END
};

static void palette_rgb(unsigned n, unsigned char *px)
{
    for (int ch = 0; ch < 3; ch++)
        px[ch] = (unsigned char)trt_sixel_palette_byte(n, ch);
}

static void fill(unsigned char *rgb, int width, int rows, int kind)
{
    unsigned char few[12][3];
    for (int k = 0; k < 12; k++)
        for (int ch = 0; ch < 3; ch++)
            few[k][ch] = (unsigned char)next_byte();
    for (long long p = 0; p < (long long)width * rows; p++)
    {
        unsigned char *px = rgb + 3 * p;
        const long long band = p / width / TRT_SIXEL_BAND;
        if (kind == FEW)
            memcpy(px, few[next_byte() % 12], 3);
        else if (kind == ONE || (kind == ALTERNATE && band % 2 == 0))
            px[0] = 255, px[1] = 0, px[2] = 9;
        else if (kind == EVERY || kind == ALTERNATE)
            palette_rgb(16u + (unsigned)(p % 240), px);
        else
            px[0] = (unsigned char)next_byte(), px[1] = (unsigned char)next_byte(), px[2] = (unsigned char)next_byte();
    }
}

/* memory with guards, and how often every byte of it was stored */
typedef struct
{
    unsigned char *bytes, *stores;
    size_t size;
    uintptr_t base; /* the address the model takes bytes[0] to have: 8-aligned */
} memory;

static void store_byte(memory *m, unsigned long long address, unsigned value)
{
    const unsigned long long at = address - m->base;
    if (address < m->base || at >= m->size)
    {
        FAIL("a store outside the memory, %lld bytes from its start", (long long)(address - m->base));
        return;
    }
    m->bytes[at] = (unsigned char)value;
    if (m->stores[at] < 255)
        m->stores[at]++;
}

static void store_word(memory *m, unsigned long long address, unsigned word)
{
    if (address & 3)
        FAIL("a word stored at an address that is %llu modulo 4", address & 3);
    for (int i = 0; i < 4; i++)
        store_byte(m, address + (unsigned)i, word >> (8 * i) & 0xffu);
}

/* the three kernels of csrc/trt_sixel.hpp; returns the length the offsets kernel stores */
static unsigned long long model(memory *m, unsigned long long out, const unsigned char *rgb, int width, int rows)
{
    const int bands = trt_sixel_bands(rows), row_bytes = trt_sixel_row_bytes(width);
    unsigned *masks = (unsigned *)calloc((size_t)bands * TRT_SIXEL_MASK_WORDS, sizeof *masks), *counts = (unsigned *)calloc((size_t)bands, sizeof *counts);
    unsigned long long *band_at = (unsigned long long *)calloc((size_t)bands, sizeof *band_at), colour_rows = 0;
    if (!masks || !counts || !band_at)
        abort();
    /* measure: a workgroup per band */
    for (int band = 0; band < bands; band++)
    {
        unsigned *mask = masks + (size_t)TRT_SIXEL_MASK_WORDS * band;
        for (int column = 0; column < width; column++)
            for (int j = 0; j < trt_sixel_band_rows(rows, band); j++)
            {
                const unsigned char *px = rgb + 3 * ((long long)(TRT_SIXEL_BAND * band + j) * width + column);
                trt_sixel_mask_set(mask, trt_xterm256_index(px[0], px[1], px[2]));
            }
        for (int w = 0; w < TRT_SIXEL_MASK_WORDS; w++)
            counts[band] += (unsigned)__builtin_popcount(mask[w]);
        if (counts[band] == 0 || counts[band] > TRT_SIXEL_COLOURS)
            FAIL("band %d of %d x %d has %u colours", band, width, rows, counts[band]);
    }
    /* offsets: the exclusive scan, the length, what stands in front of the first colour row and behind the last */
    for (int band = 0; band < bands; band++)
    {
        band_at[band] = colour_rows;
        colour_rows += counts[band];
    }
    const unsigned long long bytes = trt_sixel_text_bytes(width, colour_rows);
    for (unsigned at = 0; at < TRT_SIXEL_PROLOGUE; at++)
        store_byte(m, out + at, trt_sixel_prologue_byte(at, width, rows));
    for (unsigned e = 0; e < TRT_SIXEL_END; e++)
        store_byte(m, out + bytes - TRT_SIXEL_END + e, trt_sixel_end_byte(e));
    /* write: a thread per band and slot */
    const trt_text_split split = trt_sixel_row_split(out, width);
    const unsigned slots = trt_sixel_slots(&split);
    if (4 * split.words + split.head + split.tail != (unsigned long long)row_bytes || slots > (unsigned)row_bytes / 4 + 1)
        FAIL("the split of a colour row of %d bytes", row_bytes);
    for (int band = 0; band < bands; band++)
        for (unsigned slot = 0; slot < slots; slot++)
        {
            const int first = trt_sixel_slot_first(&split, slot);
            const int whole = first >= 0 && first + 4 <= row_bytes;
            const trt_sixel_lane lane = trt_sixel_lane_of(rgb, width, rows, band, first);
            const unsigned *mask = masks + (size_t)TRT_SIXEL_MASK_WORDS * band;
            unsigned left = counts[band];
            const int dashed = band + 1 < bands;
            unsigned long long to = out + TRT_SIXEL_PROLOGUE + (unsigned long long)row_bytes * band_at[band] + (unsigned long long)(long long)first;
            for (int w = 0; w < TRT_SIXEL_MASK_WORDS; w++)
                for (unsigned bits = mask[w]; bits; bits &= bits - 1u, to += (unsigned)row_bytes)
                {
                    const unsigned n = trt_sixel_mask_index(w, __builtin_ctz(bits));
                    left--;
                    const unsigned word = trt_sixel_lane_word(&lane, first, n, width, dashed && left == 0u);
                    if (whole)
                        store_word(m, to, word);
                    else
                        for (int i = 0; i < 4; i++)
                            if (first + i >= 0 && first + i < row_bytes)
                                store_byte(m, to + (unsigned long long)(long long)i, word >> (8 * i) & 0xffu);
                }
            if (left)
                FAIL("the walk of band %d left %u colours", band, left);
        }
    free(masks);
    free(counts);
    free(band_at);
    return bytes;
}

static void check_frame(int width, int rows, int kind)
{
    unsigned char *rgb = (unsigned char *)malloc((size_t)width * rows * 3);
    const size_t room = (size_t)trt_sixel_capacity_bytes(width, rows);
    char *want = (char *)malloc(room);
    size_t want_bytes = 0;
    if (!rgb || !want)
        abort();
    fill(rgb, width, rows, kind);
    if (trt_emitter_sixel_rgb8(rgb, width, rows, want, room, &want_bytes) != TRT_HOST_OK || want_bytes > room)
    {
        FAIL("the emitter refuses %d x %d in its capacity of %zu, or writes %zu", width, rows, room, want_bytes);
        abort();
    }
    for (unsigned offset = 0; offset < 4; offset++)
    {
        memory m;
        m.size = GUARD + 4 + room + GUARD;
        m.bytes = (unsigned char *)malloc(m.size);
        m.stores = (unsigned char *)calloc(m.size, 1);
        if (!m.bytes || !m.stores)
            abort();
        memset(m.bytes, 0xA5, m.size);
        m.base = 0x10000; /* the model's addresses are numbers: only their residues matter */
        const unsigned long long out = m.base + GUARD + offset;
        const unsigned long long bytes = model(&m, out, rgb, width, rows);
        if (bytes != want_bytes)
            FAIL("%d x %d kind %d at offset %u: %llu bytes, the emitter's text has %zu", width, rows, kind, offset, bytes, want_bytes);
        for (size_t at = 0; at < m.size; at++)
        {
            const int inside = at >= GUARD + offset && at < GUARD + offset + bytes;
            if (m.stores[at] != (inside ? 1 : 0))
            {
                FAIL("%d x %d kind %d at offset %u: byte %lld of the text stored %d times", width, rows, kind, offset, (long long)at - (long long)(GUARD + offset), m.stores[at]);
                break;
            }
        }
        if (bytes == want_bytes && memcmp(m.bytes + GUARD + offset, want, want_bytes) != 0)
        {
            size_t at = 0;
            while (m.bytes[GUARD + offset + at] == (unsigned char)want[at])
                at++;
            FAIL("%d x %d kind %d at offset %u: byte %zu is %d, the emitter's %d", width, rows, kind, offset, at, m.bytes[GUARD + offset + at], (unsigned char)want[at]);
        }
        free(m.bytes);
        free(m.stores);
    }
    free(rgb);
    free(want);
}

static void check_constants(void)
{
    static const int pads[8] = {0, 3, 2, 1, 4, 3, 2, 1}; /* T of the widths 1..7 */
    if (TRT_SIXEL_PROLOGUE != 4350 || TRT_SIXEL_FIXED != 4352)
        FAIL("the fixed bytes");
    for (int width = 1; width < 8; width++)
        if (trt_sixel_pad(width) != pads[width] || trt_sixel_row_bytes(width) % 4 != 0 || trt_sixel_row_bytes(width) != 4 + width + pads[width])
            FAIL("T or L of width %d", width);
    for (int width = 1; width <= 1030; width++)
        if (trt_sixel_pad(width) < 1 || trt_sixel_pad(width) > 4 || trt_sixel_row_bytes(width) % 4 != 0)
            FAIL("T or L of width %d", width);
    if (trt_sixel_capacity_bytes(0, 5) || trt_sixel_capacity_bytes(5, 0) || trt_sixel_capacity_bytes(-1, -1) || trt_sixel_capacity_bytes(100000, 1) ||
        trt_sixel_capacity_bytes(1, 100000) || trt_sixel_capacity_bytes(1, 1) != 4360 || trt_sixel_capacity_bytes(40, 6) != 15872 ||
        trt_sixel_capacity_bytes(40, 7) != 15872 + 48 * 40 || trt_sixel_capacity_bytes(1920, 1080) != 4352ull + 1928ull * 240 * 180 ||
        trt_sixel_capacity_bytes(99999, 99999) != 4352ull + 100004ull * 240 * 16667)
        FAIL("trt_sixel_capacity_bytes of an empty screen, above the limits or of a known size");
    static const unsigned per_cent[6] = {0, 37, 53, 69, 84, 100};
    for (unsigned level = 0; level < 6; level++)
        if (trt_sixel_percent(trt_xterm256_level_value(level)) != per_cent[level])
            FAIL("the per cent of level %u", level);
    if (trt_sixel_percent(8) != 3 || trt_sixel_percent(18) != 7 || trt_sixel_percent(238) != 93)
        FAIL("the per cent of a grey");
    for (unsigned n = 16; n < 256; n++) /* the palette's entries map to themselves but where the cube and the ramp share a colour */
    {
        const unsigned r = trt_sixel_palette_byte(n, 0), g = trt_sixel_palette_byte(n, 1), b = trt_sixel_palette_byte(n, 2);
        if (trt_xterm256_index(r, g, b) != trt_xterm256_index_search(r, g, b) || (trt_xterm256_index(r, g, b) != n && !(r == g && g == b)))
            FAIL("palette entry %u maps to %u", n, trt_xterm256_index(r, g, b));
    }
}

int main(void)
{
    static const int widths[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65, 255, 256, 257, 258, 1025}, heights[] = {1, 5, 6, 7, 13};
    check_constants();
    for (size_t i = 0; i < sizeof widths / sizeof widths[0]; i++)
        for (size_t j = 0; j < sizeof heights / sizeof heights[0]; j++)
            for (int kind = FEW; kind < KINDS_END; kind++)
                check_frame(widths[i], heights[j], kind);
    check_frame(40, 6, EVERY);
    check_frame(160, 48, FEW);
    check_frame(160, 48, ALTERNATE);
    check_frame(1, 6151, FEW);
    if (g_failures)
    {
        fprintf(stderr, "sixel_check: %d failure(s)\n", g_failures);
        return 1;
    }
    puts("sixel_check: ok");
    return 0;
}
