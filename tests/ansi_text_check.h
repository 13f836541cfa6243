/* ansi_text_check.h -- what the two check programs of the whole texts share (ansi_check.c: the full text; ansi_half_check.c: half-block cells):
 * the generator, the layout pass, the model of the wave of csrc/trt_ansi.hpp's text_write, the lane-map pass and main()'s size loops.  The position
 * map and the lane map under test are csrc/trt_text_map.h's, which the kernels compile.  A program defines its kind and includes this file once:
 *
 *   CHECK_NAME                    its name, for its messages
 *   KIND                          the format header's kind                       trt_ansi_kind()         trt_ansi_half_kind()
 *   KIND_SPAN_CELLS               the header's bound of a span's cells           TRT_ANSI_SPAN_CELLS     TRT_ANSI_HALF_SPAN_CELLS
 *   KIND_WAVE_WORDS               a wave's words, for the preprocessor
 *   KIND_TEXT_ROWS(rows)          text rows of a frame of `rows` pixel rows
 *   KIND_TEXT_BYTES(width, rows)  the header's length of the text
 *   KIND_LONE_VALUE(at, bytes)    the header's value of a lone byte
 *   KIND_MIN_BYTES                the shortest text there is (the header's claim: a tail of 3 bytes lies behind the prefix)
 *   KIND_ROWS                     layouts are checked for every width 1..70 x rows 1..KIND_ROWS
 *   KIND_MAP_ALL                  1: the lane map is checked for every such size and every larger one too; 0: for k_mapped
 *   k_larger[][2], k_mapped[][2]  larger screens for the layout pass; screens for the lane-map pass
 *   kind_held, kind_seen          what a lane holds of its cell; what a word fetches of it
 *   emitter_text()                the host emitter's text of a frame (csrc/host/trt_emit.c)
 *   kind_position_byte()          what the format header says stands at a position, the colours straight from the frame
 *   kind_hold(), kind_colours(), kind_byte()   the format's part of text_write, an array for the wave's registers and an index for the cross-lane read
 *   kind_constants()              what the kind checks of its header's constants
 *
 *  (1) layout: the text assembled position by position through trt_text_locate and the format's byte equals the emitter's; every position is
 *      classified exactly once (6 prefix bytes, every byte of every cell, the end bytes of every text row in turn, the NULs in turn); the header's
 *      length equals the emitter's; trt_text_advance from a located position and trt_text_step agree with trt_text_locate at every byte of a span,
 *      from every start a wave can have and, for small widths and for the widths either side of trt_text_advance's switch from the multiply-high to
 *      the compare, from every position; the cells of a span number at most KIND_SPAN_CELLS <= 64.
 *  (2) lane map: model_wave is text_write -- the same functions in the same order -- for batches of 1..3 frames at every residue of the output
 *      address modulo the 4-byte store, in memory with guards either side: every byte of every frame is stored exactly once, with the emitter's
 *      value, and nothing outside is stored; words are stored at aligned addresses; a word reads no lane outside the wave; the head lies in the
 *      prefix and the tail in the text's last bytes (the NULs, or the last row's end bytes).
 */
#if KIND_SPAN_CELLS > 64 || KIND_WAVE_WORDS % 64 != 0
#error "a wave's cells must fit its 64 lanes, and its words its lanes' turns"
#endif

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
            fprintf(stderr, CHECK_NAME ": " __VA_ARGS__); \
            fputc('\n', stderr);                          \
        }                                                 \
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

static char *emitter_text(int width, int rows, const unsigned char *rgb, size_t *size);
static unsigned kind_position_byte(const trt_text_at *at, int width, int rows, const unsigned char *rgb);
static kind_held kind_hold(const trt_text_at *from, int lane, int width, int rows, unsigned width_magic, const unsigned char *rgb);
/* at, last: the word's first and last byte; *rel_first, *rel_last: the cells it reads, counted from the wave's first */
static kind_seen kind_colours(const trt_text_at *at, const trt_text_at *last, const trt_text_at *from, const kind_held *mine, int width, long long *rel_first,
                              long long *rel_last);
static unsigned kind_byte(const trt_text_at *at, int rows, kind_seen shown, unsigned other);
static void kind_constants(void);

static unsigned row_magic_of(int width) { return trt_text_magic((unsigned long long)trt_text_row_bytes(KIND, width)); }

static int same_at(const trt_text_at *a, const trt_text_at *b, long long trows)
{
    if (a->r < 0 || b->r < 0 || a->row >= trows || b->row >= trows)
        return a->r == b->r && a->row == b->row;
    return a->row == b->row && a->r == b->r && a->col == b->col && a->c == b->c;
}

static void check_layout(int width, int rows, int all_starts)
{
    const trt_text_kind kind = KIND;
    const unsigned span = 4u * (unsigned)kind.wave_words;
    const long long pixels = (long long)width * rows, trows = KIND_TEXT_ROWS(rows), cells_n = trows * width;
    unsigned char *rgb = (unsigned char *)malloc((size_t)pixels * 3);
    fill_rgb(rgb, pixels);
    size_t size;
    char *want = emitter_text(width, rows, rgb, &size);
    const unsigned long long bytes = KIND_TEXT_BYTES(width, rows);
    if (bytes != size || bytes != (unsigned long long)(TRT_TEXT_HOME + kind.nuls) + (unsigned long long)(kind.cell * width + kind.end) * (unsigned long long)trows)
        FAIL("%d x %d: the header's text has %llu bytes, the emitter's %zu", width, rows, bytes, size);
    unsigned char *cells = (unsigned char *)calloc((size_t)cells_n, (size_t)kind.cell);
    long long prefix = 0, ends = 0, nuls = 0;
    for (unsigned long long t = 0; t < bytes && t < size; t++)
    {
        const trt_text_at at = trt_text_locate(kind, t, width, trows);
        const long long cell = trt_text_cell(&at, width);
        if (at.r < 0)
            prefix += at.r == (long long)t - TRT_TEXT_HOME;
        else if (at.row >= trows) /* the NULs in turn */
        {
            if (nuls >= kind.nuls || at.r != nuls || cell != cells_n)
                FAIL("%d x %d: position %llu located as byte %lld behind the last row", width, rows, t, at.r);
            nuls++;
        }
        else if (at.c >= kind.cell) /* a row's end bytes in turn, which count to its last cell */
            ends += at.col == width - 1 && at.c < kind.cell + kind.end && at.row == ends / kind.end && at.c - kind.cell == ends % kind.end;
        else if (cell < 0 || cell >= cells_n || at.c < 0 || at.col < 0 || at.col >= width || cells[cell * kind.cell + at.c]++)
            FAIL("%d x %d: position %llu classified as byte %d of cell %lld once more or out of range", width, rows, t, at.c, cell);
        const unsigned got = kind_position_byte(&at, width, rows, rgb);
        if (got != (unsigned char)want[t])
            FAIL("%d x %d: position %llu is 0x%02x, the emitter has 0x%02x", width, rows, t, got, (unsigned char)want[t]);
    }
    if (prefix != TRT_TEXT_HOME || ends != kind.end * trows || nuls != kind.nuls)
        FAIL("%d x %d: %lld prefix bytes, %lld end bytes, %lld NULs", width, rows, prefix, ends, nuls);
    for (long long i = 0; i < cells_n * kind.cell; i++)
        if (cells[i] != 1)
        {
            FAIL("%d x %d: byte %lld of cell %lld classified %d times", width, rows, i % kind.cell, i / kind.cell, cells[i]);
            break;
        }
    /* the 32-bit walk against the division, from the starts a wave can have: head + span * g -- and, where the caller asks, from every
     * position -- at every byte of the span and a little behind the text; and the cells a span touches */
    const unsigned magic = row_magic_of(width);
    for (unsigned long long start = 0; start < bytes; start += all_starts ? 1 : span)
        for (unsigned head = 0; head < (all_starts ? 1u : 4u); head++)
        {
            const trt_text_at from = trt_text_locate(kind, start + head, width, trows);
            trt_text_at walk = from;
            const long long c0 = trt_text_cell(&from, width);
            for (unsigned d = 0; d < span && start + head + d < bytes + 8; d++)
            {
                const trt_text_at direct = trt_text_locate(kind, start + head + d, width, trows), jumped = trt_text_advance(kind, &from, d, width, trows, magic);
                if (!same_at(&direct, &jumped, trows) || !same_at(&direct, &walk, trows))
                {
                    FAIL("%d x %d: %u bytes behind position %llu: located row %lld r %lld col %d c %d, advanced row %lld r %lld col %d c %d, walked row %lld r %lld col %d c %d",
                         width, rows, d, start + head, direct.row, direct.r, direct.col, direct.c, jumped.row, jumped.r, jumped.col, jumped.c, walk.row, walk.r,
                         walk.col, walk.c);
                    break;
                }
                const long long rel = trt_text_cell(&direct, width) - c0;
                if (start + head + d < bytes && (rel < 0 || rel >= KIND_SPAN_CELLS))
                {
                    FAIL("%d x %d: %u bytes behind position %llu stands cell %lld of the span, the bound is %d", width, rows, d, start + head, rel, KIND_SPAN_CELLS);
                    break;
                }
                const long long before = trt_text_cell(&walk, width);
                const int moved = trt_text_step(kind, &walk, width, trows);
                if (start + head + d + 1 < bytes - (unsigned)kind.nuls && moved != (trt_text_cell(&walk, width) != before))
                    FAIL("%d x %d: the step behind position %llu reports %d", width, rows, start + head + d, moved);
            }
        }
    free(cells);
    free(want);
    free(rgb);
}

/* text_write of csrc/trt_ansi.hpp for the 64 lanes of a wave: `mine` are its registers, stores are counted */
static void model_wave(unsigned char *memory, unsigned char *count, size_t out, int width, int rows, unsigned row_magic, unsigned width_magic, unsigned long long wave,
                       const unsigned char *rgb)
{
    const trt_text_kind kind = KIND;
    const long long trows = KIND_TEXT_ROWS(rows);
    const unsigned long long bytes = KIND_TEXT_BYTES(width, rows), tail_room = (unsigned)(kind.nuls ? kind.nuls : kind.end);
    const trt_text_split split = trt_text_split_of((unsigned long long)out, bytes);
    if (split.head > 3 || split.tail > 3 || split.head > TRT_TEXT_HOME || split.head + 4 * split.words < bytes - tail_room || split.head + 4 * split.words + split.tail != bytes)
        FAIL("%d x %d at %zu: head %u, %llu words, tail %u of %llu bytes", width, rows, out, split.head, split.words, split.tail, bytes);
    for (int lane = 0; lane < 64 && wave == 0; lane++)
    {
        const long long lone = trt_text_lone_byte(&split, lane);
        if (lone >= 0)
        {
            if (!(lone < TRT_TEXT_HOME || lone >= (long long)(bytes - tail_room)))
                FAIL("%d x %d: the lone byte %lld lies neither in the prefix nor in the last %llu bytes", width, rows, lone, tail_room);
            memory[out + lone] = (unsigned char)KIND_LONE_VALUE(lone, bytes), count[out + lone]++;
        }
    }
    const unsigned long long first = trt_text_lane_word(kind, wave, 0, 0);
    if (first >= split.words)
        return;
    const trt_text_at from = trt_text_locate(kind, split.head + 4 * first, width, trows);
    kind_held mine[64];
    for (int lane = 0; lane < 64; lane++)
        mine[lane] = kind_hold(&from, lane, width, rows, width_magic, rgb);
    for (int j = 0; j < KIND_WAVE_WORDS / 64; j++)
        for (int lane = 0; lane < 64; lane++)
        {
            const unsigned long long k = trt_text_lane_word(kind, wave, lane, j);
            trt_text_at at[4];
            unsigned other[4] = {0u};
            at[0] = trt_text_advance(kind, &from, 4u * (unsigned)(64 * j + lane), width, trows, row_magic);
            for (int b = 1; b < 4; b++)
            {
                at[b] = at[b - 1];
                other[b] = other[b - 1] | (unsigned)trt_text_step(kind, &at[b], width, trows);
            }
            long long rel_first, rel_last;
            const kind_seen shown = kind_colours(&at[0], &at[3], &from, mine, width, &rel_first, &rel_last);
            if (k < split.words && (rel_first < 0 || rel_last > 63) && at[0].row < trows)
                FAIL("%d x %d: word %llu reads the cells %lld and %lld behind its wave's first", width, rows, k, rel_first, rel_last);
            unsigned word = 0;
            for (int b = 0; b < 4; b++)
                word |= kind_byte(&at[b], rows, shown, other[b]) << (8 * b);
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
    const trt_text_kind kind = KIND;
    const long long pixels = (long long)width * rows;
    const unsigned long long bytes = KIND_TEXT_BYTES(width, rows);
    const unsigned row_magic = row_magic_of(width), width_magic = trt_text_magic((unsigned long long)width);
    enum { GUARD = 64 };
    if (bytes < KIND_MIN_BYTES)
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
            const unsigned long long waves = trt_text_waves(kind, frames > 1 ? bytes / 4 : trt_text_split_of(GUARD + offset, bytes).words);
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

/* a width either side of trt_text_advance's switch: rows one cell shorter are below a span, rows one cell longer are not */
static int at_the_switch(int width)
{
    const trt_text_kind kind = KIND;
    return (trt_text_row_bytes(kind, width - 1) >= 4 * kind.wave_words) != (trt_text_row_bytes(kind, width + 1) >= 4 * kind.wave_words);
}

int main(void)
{
    kind_constants();
    if (TRT_TEXT_SPAN_CELLS(KIND.cell, KIND.wave_words) != KIND_SPAN_CELLS || KIND.wave_words != KIND_WAVE_WORDS || KIND.end > KIND.cell)
        FAIL("a span of %d bytes touches up to %d cells", 4 * KIND.wave_words, KIND_SPAN_CELLS);
    for (int width = 1; width <= 70; width++)
        for (int rows = 1; rows <= KIND_ROWS; rows++)
        {
            check_layout(width, rows, width <= 6 || at_the_switch(width));
            if (KIND_MAP_ALL)
                check_lane_map(width, rows);
        }
    for (size_t i = 0; i < sizeof k_larger / sizeof k_larger[0]; i++)
    {
        check_layout(k_larger[i][0], k_larger[i][1], 0);
        if (KIND_MAP_ALL)
            check_lane_map(k_larger[i][0], k_larger[i][1]);
    }
    for (size_t i = 0; i < sizeof k_mapped / sizeof k_mapped[0]; i++)
        check_lane_map(k_mapped[i][0], k_mapped[i][1]);
    for (int ch = 0; ch < 3; ch++)
        for (int v = 0; v < 256; v++)
            if (!g_seen[ch][v])
                FAIL("channel %d never took the value %d", ch, v);
    if (g_failures)
    {
        fprintf(stderr, CHECK_NAME ": %d failure(s)\n", g_failures);
        return 1;
    }
    puts(CHECK_NAME ": ok");
    return 0;
}
