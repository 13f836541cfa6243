/* xterm256_check.c -- csrc/trt_xterm256.h, the closed form of a colour's entry in the xterm 256-colour palette that the device kernels compute,
 * compiled for the host and held against the rule itself: trt_xterm256_index_search (csrc/host/trt_emit.c), the loop over the 240 fixed entries
 * that keeps the first of the nearest.  A program of its own: tests/test_xterm256_map.py builds and runs it plain, on every colour, and under
 * -fsanitize=address,undefined on every `step`-th colour (the argument; 1 without one).
 *
 *  (1) the closed form equals the search on the colours 0, step, 2 step, ... < 2^24 (r the low byte);
 *  (2) the known answers: the corners, the greys between cube levels, the ties (cube against ramp: the cube, the lower index; ramp against ramp:
 *      the lower step) and the ramp's end;
 *  (3) with step 1: every index 16..255 occurs; with any step: none below 16 or above 255.
 */
#include <stdio.h>
#include <stdlib.h>

#include "trt_xterm256.h" /* in front of trt_host.h: trt_xterm256_index is this header's inline function here */

#include "trt_host.h"

static int g_failures;
#define FAIL(...)                                        \
    do                                                   \
    {                                                    \
        if (g_failures++ < 20)                           \
        {                                                \
            fprintf(stderr, "xterm256_check: " __VA_ARGS__); \
            fputc('\n', stderr);                         \
        }                                                \
    } while (0)

static const struct
{
    unsigned r, g, b, index;
} k_known[] = {
    {0, 0, 0, 16},       {255, 255, 255, 231}, {128, 128, 128, 244}, {115, 115, 115, 243}, {47, 48, 115, 238},
    {4, 4, 4, 16},       /* as far from black as from the grey 8: the lower index */
    {5, 5, 5, 232},      {13, 13, 13, 232},    /* between the greys 8 and 18: the lower */
    {246, 246, 246, 255}, {247, 247, 247, 231},
    {255, 0, 0, 196},    {0, 255, 0, 46},      {0, 0, 255, 21},      {95, 135, 175, 67},   {8, 8, 8, 232},   {238, 238, 238, 255},
};

int main(int argc, char **argv)
{
    const unsigned long step = argc > 1 ? strtoul(argv[1], NULL, 10) : 1;
    if (step == 0)
        return 2;
    static unsigned long occurs[256];
    for (unsigned long colour = 0; colour < 1ul << 24; colour += step)
    {
        const unsigned r = colour & 0xff, g = (colour >> 8) & 0xff, b = colour >> 16;
        const unsigned got = trt_xterm256_index(r, g, b), want = trt_xterm256_index_search(r, g, b);
        if (got != want)
            FAIL("(%u, %u, %u): the closed form gives %u, the search %u", r, g, b, got, want);
        if (got != trt_xterm256_index_of(r | g << 8 | b << 16))
            FAIL("(%u, %u, %u): the packed form differs", r, g, b);
        occurs[got & 0xff]++;
        if (got > 255)
            FAIL("(%u, %u, %u): index %u", r, g, b, got);
    }
    for (unsigned index = 0; index < 256; index++)
    {
        if (index < 16 && occurs[index])
            FAIL("index %u, which is the user's to theme, occurs %lu times", index, occurs[index]);
        if (index >= 16 && step == 1 && !occurs[index])
            FAIL("index %u never occurs", index);
    }
    for (size_t i = 0; i < sizeof k_known / sizeof k_known[0]; i++)
    {
        const unsigned closed = trt_xterm256_index(k_known[i].r, k_known[i].g, k_known[i].b), search = trt_xterm256_index_search(k_known[i].r, k_known[i].g, k_known[i].b);
        if (closed != k_known[i].index || search != k_known[i].index)
            FAIL("(%u, %u, %u) is %u: the closed form gives %u, the search %u", k_known[i].r, k_known[i].g, k_known[i].b, k_known[i].index, closed, search);
    }
    if (TRT_XTERM256_BLACK != 16 || trt_xterm256_index(0, 0, 0) != TRT_XTERM256_BLACK || TRT_XTERM256_FIRST != 16 || TRT_XTERM256_GREYS != 232)
        FAIL("the header's constants");
    if (g_failures)
    {
        fprintf(stderr, "xterm256_check: %d failure(s)\n", g_failures);
        return 1;
    }
    puts("xterm256_check: ok");
    return 0;
}
