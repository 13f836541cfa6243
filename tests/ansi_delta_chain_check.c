/* ansi_delta_chain_check.c -- csrc/trt_ansi_delta_chain.h, a chain of n delta texts as one prefix sum over the tiles of n pairs of frames,
 * compiled for the host and held against the sequential emitters of csrc/host/trt_emit.c, one pair at a time.  A program of its own, one per
 * kind of cell: the full text's as it stands, half-block cells with -DCHAIN_HALF; tests/test_ansi_delta_batch_layout.py builds and runs both
 * plain and under -fsanitize=address,undefined.
 *
 * check() goes about a chain as the device does (csrc/trt_ansi_delta.hpp): for every pair b, every tile and every thread 0 ..
 * TRT_DELTA_BLOCK - 1 it calls the kind's own lane walk on the two frames trt_delta_chain_frames names and sums the lanes' totals into
 * entry trt_delta_chain_tile of the sums (measure, a grid of tiles x n); scans all n * tiles sums exclusively from `base` in turns of
 * TRT_DELTA_SCAN_BLOCK with a running total, frame boundaries wherever they fall, and takes the n lengths from the offsets by
 * trt_delta_chain_text_bytes (offsets); and places each lane at its tile's offset plus the totals of the lanes before it (write), into one
 * buffer with a count per byte.  Every text and every length is the emitter's of its two frames, text b starts at base plus the lengths
 * before it, every byte from base to the total was stored exactly once, none below base and none at or behind the total.
 *
 * Allocation is to the byte: the n frames are ONE allocation of exactly n * rows * width * 3 bytes, the shown frame one of its own, so a
 * load behind the last frame, or in front of the first, is the address sanitizer's to report; a load behind any other frame -- a lower row
 * of an odd frame in half-block cells -- reads the next frame, which differs, and the text is no longer the emitter's.
 *
 * Chains: n in {1, 2, 3, 8}; 1x1, 1x3, 2x1, 63x2, 64x3, 65x5, 160x47; steps from one frame to the next that cycle, from every starting point,
 * through: equal frames (a text of 0 bytes, in the middle of a chain too), every cell changed with all neighbours different, 40 % changed,
 * back to the frame before last, the first cell only, the last cell only.  And one chain of more than 1024 tiles in all, so that frames begin
 * inside a turn of the scan: n = 8 at 2047x65 (130 tiles a frame, 1040) for the full text's cells, at 2047x131 (132, 1056) for half-block cells.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trt_ansi_delta_chain.h"
#include "trt_ansi_delta_half.h"
#include "trt_host.h"

#ifdef CHAIN_HALF
#define CHECK_NAME "ansi_delta_half_chain_check"
#define KIND_LANE trt_delta_half_lane
#define KIND_LANE_CELLS trt_delta_half_lane_cells
#define KIND_LANE_BYTE trt_delta_half_lane_byte
#define KIND_EMITTER trt_emitter_delta_half_rgb8
#define KIND_BOUND trt_delta_half_bound
#define KIND_TEXT_ROWS(rows) trt_ansi_half_text_rows(rows)
#define LARGE_ROWS 131
#define LARGE_TILES 132
#else
#define CHECK_NAME "ansi_delta_chain_check"
#define KIND_LANE trt_delta_lane
#define KIND_LANE_CELLS trt_delta_lane_cells
#define KIND_LANE_BYTE trt_delta_lane_byte
#define KIND_EMITTER trt_emitter_delta_rgb8
#define KIND_BOUND trt_delta_bound
#define KIND_TEXT_ROWS(rows) (rows)
#define LARGE_ROWS 65
#define LARGE_TILES 130
#endif

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_random(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 40);
}

static int g_failures;
static long g_cases, g_empty_inside;
#define FAIL(...)                                         \
    do                                                    \
    {                                                     \
        if (g_failures++ < 20)                            \
        {                                                 \
            fprintf(stderr, CHECK_NAME ": " __VA_ARGS__); \
            fputc('\n', stderr);                          \
        }                                                 \
    } while (0)

static void put(unsigned char *frame, long long p, unsigned rgb)
{
    frame[3 * p] = (unsigned char)rgb, frame[3 * p + 1] = (unsigned char)(rgb >> 8), frame[3 * p + 2] = (unsigned char)(rgb >> 16);
}
static unsigned get(const unsigned char *frame, long long p) { return (unsigned)frame[3 * p] | (unsigned)frame[3 * p + 1] << 8 | (unsigned)frame[3 * p + 2] << 16; }

/* a colour that is neither `a` nor `b` */
static unsigned other_than(unsigned a, unsigned b)
{
    unsigned c;
    do
        c = next_random() & 0xffffffu;
    while (c == a || c == b);
    return c;
}

enum
{
    EQUAL,         /* nothing changed: a text of 0 bytes */
    ALL_DIFFERENT, /* every pixel changed, all horizontal neighbours different */
    FORTY,         /* 40 % of the pixels changed */
    BACK,          /* the frame before last again */
    FIRST_ONLY,
    LAST_ONLY,
    STEPS
};

/* frame `next` from frame `last`; before_last: the frame in front of `last`, NULL where the chain has none yet */
static void step(int kind, int width, int rows, const unsigned char *before_last, const unsigned char *last, unsigned char *next)
{
    const long long pixels = (long long)width * rows;
    memcpy(next, last, (size_t)pixels * 3);
    if (kind == BACK && !before_last) /* a chain's first step has no frame before last */
        kind = FORTY;
    switch (kind)
    {
    case EQUAL:
        break;
    case ALL_DIFFERENT:
        for (long long p = 0; p < pixels; p++)
            put(next, p, other_than(get(last, p), p % width ? get(next, p - 1) : get(last, p)));
        break;
    case BACK:
        memcpy(next, before_last, (size_t)pixels * 3);
        break;
    case FORTY:
        for (long long p = 0; p < pixels; p++)
            if ((next_random() & 0xffffffu) < 6710886u) /* 0.4 of 2^24 */
                put(next, p, other_than(get(last, p), get(last, p)));
        break;
    case FIRST_ONLY:
        put(next, 0, other_than(get(last, 0), get(last, 0)));
        break;
    default:
        put(next, pixels - 1, other_than(get(last, pixels - 1), get(last, pixels - 1)));
        break;
    }
}

/* a chain of n frames of width x rows whose steps are start, start + 1 ... modulo STEPS; the texts stand behind `base` bytes */
static void check(int width, int rows, unsigned n, int start, unsigned long long base)
{
    const size_t frame_bytes = (size_t)width * rows * 3;
    const unsigned long long cells = (unsigned long long)width * KIND_TEXT_ROWS(rows), tiles = trt_delta_tiles(cells), bound = KIND_BOUND(width, rows);
    const unsigned long long capacity = base + n * bound;
    unsigned char *shown = (unsigned char *)malloc(frame_bytes), *frames = (unsigned char *)malloc(n * frame_bytes); /* to the byte */
    char *want = (char *)malloc((size_t)capacity);
    size_t want_bytes[TRT_DELTA_CHAIN_MAX];
    unsigned char *got = (unsigned char *)calloc((size_t)capacity + 64, 1), *stores = (unsigned char *)calloc((size_t)capacity + 64, 1);
    unsigned *tile_bytes = (unsigned *)calloc((size_t)(n * tiles), sizeof *tile_bytes);
    unsigned long long *tile_at = (unsigned long long *)calloc((size_t)(n * tiles), sizeof *tile_at);
    g_cases++;
    if (trt_delta_chain_stride(width, rows) != frame_bytes)
        FAIL("%d x %d: a frame stride of %llu", width, rows, trt_delta_chain_stride(width, rows));
    for (long long p = 0; p < (long long)width * rows; p++)
        put(shown, p, next_random() & 0xffffffu);
    for (unsigned b = 0; b < n; b++)
        step((start + (int)b) % STEPS, width, rows, b == 0 ? NULL : b == 1 ? shown : frames + (b - 2) * frame_bytes, b == 0 ? shown : frames + (b - 1) * frame_bytes,
             frames + b * frame_bytes);
    /* the emitter, pair by pair, back to back behind `base` */
    unsigned long long want_total = base;
    for (unsigned b = 0; b < n; b++)
    {
        const unsigned char *from = b == 0 ? shown : frames + (b - 1) * frame_bytes;
        if (KIND_EMITTER(from, frames + b * frame_bytes, width, rows, want + want_total, (size_t)bound, &want_bytes[b]) != TRT_HOST_OK)
            FAIL("%d x %d: the emitter refused pair %u", width, rows, b);
        want_total += want_bytes[b];
        if (want_bytes[b] == 0 && b > 0 && b + 1 < n)
            g_empty_inside++;
    }
    /* measure: a grid of tiles x n */
    for (unsigned b = 0; b < n; b++)
    {
        const trt_delta_chain_pair pair = trt_delta_chain_frames(shown, frames, width, rows, b);
        for (unsigned long long t = 0; t < tiles; t++)
            for (unsigned thread = 0; thread < TRT_DELTA_BLOCK; thread++)
                tile_bytes[trt_delta_chain_tile(tiles, b, t)] += KIND_LANE_CELLS(pair.shown, pair.next, width, rows, t, thread).total;
    }
    /* offsets: ONE scan over all n * tiles sums from `base`, turns of TRT_DELTA_SCAN_BLOCK and a running total; then the n lengths */
    unsigned long long running = base;
    for (unsigned long long first = 0; first < n * tiles; first += TRT_DELTA_SCAN_BLOCK)
    {
        unsigned long long turn = 0;
        for (unsigned long long i = first; i < first + TRT_DELTA_SCAN_BLOCK && i < n * tiles; i++)
            tile_at[i] = running + turn, turn += tile_bytes[i];
        running += turn;
    }
    unsigned long long before = base;
    for (unsigned b = 0; b < n; b++)
    {
        const unsigned long long length = trt_delta_chain_text_bytes(tile_at, tiles, n, b, running), at = trt_delta_chain_text_at(tile_at, tiles, b);
        if (length != want_bytes[b])
            FAIL("%d x %d, n = %u from step %d: text %u has %llu bytes through the header, %zu from the emitter", width, rows, n, start, b, length, want_bytes[b]);
        if (at != before)
            FAIL("%d x %d, n = %u from step %d: text %u starts at %llu, the texts before it end at %llu", width, rows, n, start, b, at, before);
        before += want_bytes[b];
    }
    /* write: the same grid; every lane behind the totals of the lanes before it, its records in order; the capacity is the whole buffer's */
    for (unsigned b = 0; b < n; b++)
    {
        const trt_delta_chain_pair pair = trt_delta_chain_frames(shown, frames, width, rows, b);
        for (unsigned long long t = 0; t < tiles; t++)
        {
            unsigned long long at = tile_at[trt_delta_chain_tile(tiles, b, t)];
            for (unsigned thread = 0; thread < TRT_DELTA_BLOCK; thread++)
            {
                const KIND_LANE lane = KIND_LANE_CELLS(pair.shown, pair.next, width, rows, t, thread);
                for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
                {
                    if (at + lane.bytes[j] > capacity)
                        FAIL("%d x %d, n = %u: a record behind the capacity", width, rows, n);
                    else
                        for (unsigned k = 0; k < lane.bytes[j]; k++)
                            got[at + k] = (unsigned char)KIND_LANE_BYTE(&lane, j, k), stores[at + k]++;
                    at += lane.bytes[j];
                }
            }
        }
    }
    if (running != want_total)
        FAIL("%d x %d, n = %u from step %d: %llu bytes in all through the header, %llu from the emitter", width, rows, n, start, running, want_total);
    else if (memcmp(got + base, want + base, (size_t)(want_total - base)) != 0)
    {
        size_t at = (size_t)base;
        while (got[at] == (unsigned char)want[at])
            at++;
        FAIL("%d x %d, n = %u from step %d: the texts differ from byte %zu of %llu", width, rows, n, start, at, want_total);
    }
    for (unsigned long long i = 0; i < capacity + 64; i++)
        if (stores[i] != (i >= base && i < running ? 1 : 0))
        {
            FAIL("%d x %d, n = %u from step %d: byte %llu of [%llu, %llu) stored %d times", width, rows, n, start, i, base, running, stores[i]);
            break;
        }
    free(shown), free(frames), free(want), free(got), free(stores), free(tile_bytes), free(tile_at);
}

int main(void)
{
    static const int k_sizes[][2] = {{1, 1}, {1, 3}, {2, 1}, {63, 2}, {64, 3}, {65, 5}, {160, 47}};
    static const unsigned k_n[] = {1, 2, 3, 8};
    if (TRT_DELTA_CHAIN_MAX != 8 || TRT_DELTA_SCAN_BLOCK != 1024)
        FAIL("the constants");
    for (size_t s = 0; s < sizeof k_sizes / sizeof k_sizes[0]; s++)
        for (size_t i = 0; i < sizeof k_n / sizeof k_n[0]; i++)
            for (int start = 0; start < STEPS; start++)
                check(k_sizes[s][0], k_sizes[s][1], k_n[i], start, start & 1 ? 0 : 77ull * (unsigned)start); /* behind a keyframe's bytes, too */
    if (g_empty_inside == 0)
        FAIL("no chain had a text of 0 bytes in its middle");
    /* more than one turn of the scan: frames begin inside a turn */
    if (trt_delta_tiles(2047ull * KIND_TEXT_ROWS(LARGE_ROWS)) != LARGE_TILES || 8 * LARGE_TILES <= TRT_DELTA_SCAN_BLOCK || TRT_DELTA_SCAN_BLOCK % LARGE_TILES == 0)
        FAIL("the large chain has %llu tiles a frame", trt_delta_tiles(2047ull * KIND_TEXT_ROWS(LARGE_ROWS)));
    check(2047, LARGE_ROWS, 8, 1, 0);
    check(2047, LARGE_ROWS, 8, 4, 12345);
    if (g_failures)
    {
        fprintf(stderr, CHECK_NAME ": %d failure(s)\n", g_failures);
        return 1;
    }
    printf(CHECK_NAME ": ok (%ld cases)\n", g_cases);
    return 0;
}
