/* ansi256_delta_check.h -- what the two check programs of the delta texts in the xterm 256-colour palette share (ansi256_delta_check.c: the
 * full text's cells; ansi256_delta_half_check.c: half-block cells): the generator, the families of frame pairs, check(), which assembles a
 * pair's text THROUGH THE KERNELS' OWN WALK and holds it against the sequential emitter, and the enumeration of a row's longest text.  A
 * program defines its kind as for ansi_delta_check.h -- CHECK_NAME, KIND_LANE, KIND_LANE_CELLS, KIND_LANE_BYTE, KIND_EMITTER, KIND_BOUND,
 * KIND_TEXT_ROWS, KIND_RECORD_MAX, k_lengths[], LENGTHS, kind_verdicts() -- and includes this file once.
 *
 * The families are those of ansi_delta_check.h (and of tests/ansi_delta_support.py), each in two MODES -- colours of any bytes, where a
 * changed byte need not change the index, and colours that are entries of the palette, where "different" means a different index -- and
 * three that only a palette text has:
 *
 *   SAME_INDEX   every pixel's bytes differ between the frames and no index does, neighbours of different indices: no text at all, where the
 *                24-bit delta text is at its bound
 *   INDEX_RUN    every cell changed, a row's new colours of alternating bytes and ONE index: the colour stands at the run's start alone
 *   LONGEST      the pattern the bound is reached by (full cells: changed and unchanged cells in turn; half-block cells: every cell changed,
 *                both indices different from the left neighbour's)
 *
 * check() goes about it as the device does (csrc/trt_ansi_delta.hpp), exactly as ansi_delta_check.h's: measure, offsets in turns of
 * TRT_DELTA_SCAN_BLOCK, write into a buffer with a count per byte.  The frames are allocated at exactly rows * width * 3 bytes: a load
 * behind a frame is the address sanitizer's to report.
 */
static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned next_random(void)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_state >> 40);
}

static int g_failures;
static long g_cases;
#define FAIL(...)                                        \
    do                                                   \
    {                                                    \
        if (g_failures++ < 20)                           \
        {                                                \
            fprintf(stderr, CHECK_NAME ": " __VA_ARGS__); \
            fputc('\n', stderr);                         \
        }                                                \
    } while (0)

enum
{
    NOTHING,
    ALL_DIFFERENT, /* every pixel changed, all horizontal neighbours different */
    ALL_ONE,       /* every pixel changed, one colour */
    ALTERNATE,     /* every other pixel */
    FIRST_ONLY,
    LAST_ONLY,
    ACROSS_ROWS, /* a run into a pixel row's last cell, one from the next row's first cell, the same colour */
    LEFT_COLOUR, /* a changed pixel whose new colour is its unchanged left neighbour's */
    RANDOM_TWO_001, RANDOM_TWO_40, RANDOM_TWO_99, RANDOM_FULL_001, RANDOM_FULL_40, RANDOM_FULL_99,
    UPPER_ONLY, /* only the even pixel rows changed */
    LOWER_ONLY, /* only the odd ones */
    SAME_UPPER, /* every pixel changed, the even rows to one colour while the odd rows' neighbours differ */
    SAME_LOWER, /* the converse */
    SAME_INDEX,
    INDEX_RUN,
    LONGEST,
    ALL_FAMILIES
};
static const char *const k_family[ALL_FAMILIES] = {"nothing", "all different", "all one colour", "alternate", "first only", "last only", "across rows", "left colour",
                                                   "random two 0.01", "random two 0.4", "random two 0.99", "random full 0.01", "random full 0.4", "random full 0.99",
                                                   "upper only", "lower only", "same upper", "same lower", "same index", "index run", "longest"};
static unsigned g_seen[ALL_FAMILIES]; /* bit i: a record of k_lengths[i] bytes occurred */
static int g_entries;                 /* the mode: colours are entries of the palette */

static void kind_verdicts(int family, int width, int rows, unsigned long long length, unsigned long long bound, const unsigned char *shown, const unsigned char *next);
static void kind_longest(unsigned char *shown, unsigned char *next, int width, int rows); /* the LONGEST family's frames, over random ones */
static unsigned kind_cell_bytes(int changed_left, int state, int changed_right);           /* for the enumeration, below */

static void put(unsigned char *frame, long long p, unsigned rgb)
{
    frame[3 * p] = (unsigned char)rgb, frame[3 * p + 1] = (unsigned char)(rgb >> 8), frame[3 * p + 2] = (unsigned char)(rgb >> 16);
}
static unsigned get(const unsigned char *frame, long long p) { return (unsigned)frame[3 * p] | (unsigned)frame[3 * p + 1] << 8 | (unsigned)frame[3 * p + 2] << 16; }
static unsigned index_of(unsigned rgb) { return trt_xterm256_index_search(rgb & 0xffu, (rgb >> 8) & 0xffu, (rgb >> 16) & 0xffu); }

/* the colour of palette entry 16..255, r | g << 8 | b << 16 */
static unsigned entry_colour(unsigned index)
{
    static const unsigned levels[6] = {0, 95, 135, 175, 215, 255};
    if (index >= 232)
        return (8 + 10 * (index - 232)) * 0x010101u;
    index -= 16;
    return levels[index / 36] | levels[index / 6 % 6] << 8 | levels[index % 6] << 16;
}
/* other bytes of the same index: the red byte one off.  The levels and the greys are far enough apart for that, which make_frames holds
 * against the search */
static unsigned nudged(unsigned rgb) { return (rgb & 0xffu) == 255u ? rgb - 1u : rgb + 1u; }

static unsigned any_colour(void) { return g_entries ? entry_colour(16 + next_random() % 240) : next_random() & 0xffffffu; }

/* a colour that is neither `a` nor `b`: in the palette mode of another index than both */
static unsigned other_than(unsigned a, unsigned b)
{
    unsigned c;
    do
        c = any_colour();
    while (c == a || c == b || (g_entries && (index_of(c) == index_of(a) || index_of(c) == index_of(b))));
    return c;
}

static void row_all_different(const unsigned char *shown, unsigned char *next, int width, int r)
{
    for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
        put(next, p, other_than(get(shown, p), p % width ? get(next, p - 1) : get(shown, p)));
}
static void row_all_one(unsigned char *shown, unsigned char *next, int width, int r)
{
    for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
        put(shown, p, 0x102030u + (unsigned)(p & 1)), put(next, p, 0xa0b0c0u);
}

static void make_frames(int family, int width, int rows, unsigned char *shown, unsigned char *next)
{
    const long long pixels = (long long)width * rows;
    for (long long p = 0; p < pixels; p++)
        put(shown, p, any_colour());
    memcpy(next, shown, (size_t)pixels * 3);
    switch (family)
    {
    case NOTHING:
        break;
    case ALL_DIFFERENT:
        for (int r = 0; r < rows; r++)
            row_all_different(shown, next, width, r);
        break;
    case ALL_ONE:
        for (int r = 0; r < rows; r++)
            row_all_one(shown, next, width, r);
        break;
    case UPPER_ONLY:
        for (int r = 0; r < rows; r += 2)
            row_all_different(shown, next, width, r);
        break;
    case LOWER_ONLY:
        for (int r = 1; r < rows; r += 2)
            row_all_different(shown, next, width, r);
        break;
    case SAME_UPPER:
    case SAME_LOWER:
        for (int r = 0; r < rows; r++)
            if ((r & 1) == (family == SAME_LOWER))
                row_all_one(shown, next, width, r);
            else
                row_all_different(shown, next, width, r);
        break;
    case ALTERNATE:
        for (long long p = 0; p < pixels; p += 2)
            put(next, p, other_than(get(shown, p), get(shown, p)));
        break;
    case FIRST_ONLY:
        put(next, 0, other_than(get(shown, 0), get(shown, 0)));
        break;
    case LAST_ONLY:
        put(next, pixels - 1, other_than(get(shown, pixels - 1), get(shown, pixels - 1)));
        break;
    case ACROSS_ROWS:
        for (int r = 0; r + 1 < rows || r == 0; r++)
        { /* the last two pixels of row r (where there are two) and the first two of row r + 1 */
            for (int c = width > 1 ? width - 2 : 0; c < width; c++)
                put(shown, (long long)r * width + c, 0x010101u), put(next, (long long)r * width + c, 0x00ff7fu);
            if (r + 1 < rows)
                for (int c = 0; c < 2 && c < width; c++)
                    put(shown, (long long)(r + 1) * width + c, 0x020202u), put(next, (long long)(r + 1) * width + c, 0x00ff7fu);
        }
        break;
    case LEFT_COLOUR:
        for (long long p = 1; p < pixels; p += 3)
            if (get(shown, p) != get(shown, p - 1))
                put(next, p, get(next, p - 1));
        break;
    case SAME_INDEX: /* entries, neighbours of different indices; the next frame one byte off every pixel */
        for (long long p = 0; p < pixels; p++)
        {
            unsigned index;
            do
                index = 16 + next_random() % 240;
            while (p % width && index == index_of(get(shown, p - 1)));
            put(shown, p, entry_colour(index));
            put(next, p, nudged(entry_colour(index)));
            if (index_of(get(next, p)) != index || get(next, p) == get(shown, p))
                FAIL("same index: %06x is no other colour of entry %u", get(next, p), index);
        }
        break;
    case INDEX_RUN: /* a pixel row goes from one entry to another, the new bytes of neighbours one off */
        for (int r = 0; r < rows; r++)
        {
            const unsigned from = 16 + next_random() % 240, to = 16 + (from - 16 + 1 + next_random() % 239) % 240;
            for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
                put(shown, p, entry_colour(from)), put(next, p, p & 1 ? nudged(entry_colour(to)) : entry_colour(to));
            if (index_of(nudged(entry_colour(to))) != to || from == to)
                FAIL("index run: entries %u and %u", from, to);
        }
        break;
    case LONGEST:
        kind_longest(shown, next, width, rows);
        break;
    default:
    {
        const int two = family < RANDOM_FULL_001;
        const int which = (family - RANDOM_TWO_001) % 3;
        const unsigned threshold = which == 0 ? 167772u : which == 1 ? 6710886u : 16609443u; /* 0.01, 0.4, 0.99 of 2^24 */
        if (two)
            for (long long p = 0; p < pixels; p++)
                put(shown, p, next_random() & 1 ? 0xffffffu : 0x000000u);
        memcpy(next, shown, (size_t)pixels * 3);
        for (long long p = 0; p < pixels; p++)
            if ((next_random() & 0xffffffu) < threshold)
                put(next, p, two ? get(shown, p) ^ 0xffffffu : other_than(get(shown, p), get(shown, p)));
        break;
    }
    }
}

static unsigned long long check(int family, int width, int rows)
{
    const long long pixels = (long long)width * rows, cells = (long long)width * KIND_TEXT_ROWS(rows);
    const unsigned long long bound = KIND_BOUND(width, rows), tiles = trt_delta_tiles((unsigned long long)cells);
    unsigned char *shown = (unsigned char *)malloc((size_t)pixels * 3), *next = (unsigned char *)malloc((size_t)pixels * 3); /* to the byte */
    char *want = (char *)malloc((size_t)bound);
    unsigned char *got = (unsigned char *)calloc((size_t)bound + 64, 1), *stores = (unsigned char *)calloc((size_t)bound + 64, 1);
    unsigned *tile_bytes = (unsigned *)calloc((size_t)tiles, sizeof *tile_bytes);
    unsigned long long *tile_at = (unsigned long long *)calloc((size_t)tiles, sizeof *tile_at);
    size_t want_bytes = 0;
    g_cases++;
    make_frames(family, width, rows, shown, next);
    if (KIND_EMITTER(shown, next, width, rows, want, (size_t)bound, &want_bytes) != TRT_HOST_OK)
        FAIL("%s %d x %d: the emitter refused", k_family[family], width, rows);
    if (KIND_EMITTER(shown, next, width, rows, want, (size_t)bound - 1, &want_bytes) != TRT_HOST_ERR_ARGUMENT)
        FAIL("%d x %d: the emitter took a capacity below the bound", width, rows);
    /* measure: the lanes' totals, a sum per tile */
    for (unsigned long long t = 0; t < tiles; t++)
    {
        for (unsigned thread = 0; thread < TRT_DELTA_BLOCK; thread++)
        {
            const KIND_LANE lane = KIND_LANE_CELLS(shown, next, width, rows, t, thread);
            unsigned total = 0;
            for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
            {
                const unsigned n = lane.bytes[j];
                int known = n == 0;
                for (int i = 0; i < LENGTHS; i++)
                    if (n == k_lengths[i])
                        known = 1, g_seen[family] |= 1u << i;
                if (!known)
                    FAIL("%s %d x %d: a record of %u bytes at cell %d of thread %u of tile %llu", k_family[family], width, rows, n, j, thread, t);
                total += n;
            }
            if (total != lane.total)
                FAIL("%s %d x %d: thread %u of tile %llu: a total of %u for records of %u bytes", k_family[family], width, rows, thread, t, lane.total, total);
            tile_bytes[t] += lane.total;
        }
        if (tile_bytes[t] > TRT_DELTA_TILE * KIND_RECORD_MAX)
            FAIL("%s %d x %d: tile %llu has %u bytes", k_family[family], width, rows, t, tile_bytes[t]);
    }
    /* offsets: turns of TRT_DELTA_SCAN_BLOCK sums, a running total */
    unsigned long long running = 0;
    for (unsigned long long first = 0; first < tiles; first += TRT_DELTA_SCAN_BLOCK)
    {
        unsigned long long turn = 0;
        for (unsigned long long t = first; t < first + TRT_DELTA_SCAN_BLOCK && t < tiles; t++)
            tile_at[t] = running + turn, turn += tile_bytes[t];
        running += turn;
    }
    const unsigned long long length = running;
    /* write: per tile, every lane behind the totals of the lanes before it, its records in order */
    for (unsigned long long t = 0; t < tiles; t++)
    {
        unsigned long long at = tile_at[t];
        for (unsigned thread = 0; thread < TRT_DELTA_BLOCK; thread++)
        {
            const KIND_LANE lane = KIND_LANE_CELLS(shown, next, width, rows, t, thread);
            for (int j = 0; j < TRT_DELTA_LANE_CELLS; j++)
            {
                for (unsigned k = 0; k < lane.bytes[j]; k++)
                {
                    if (at + k >= bound)
                    {
                        FAIL("%s %d x %d: a store behind the bound", k_family[family], width, rows);
                        break;
                    }
                    got[at + k] = (unsigned char)KIND_LANE_BYTE(&lane, j, k);
                    stores[at + k]++;
                }
                at += lane.bytes[j];
            }
        }
    }
    if (length != want_bytes)
        FAIL("%s %d x %d: %llu bytes through the header, %zu from the emitter", k_family[family], width, rows, length, want_bytes);
    else if (memcmp(got, want, want_bytes) != 0)
    {
        size_t at = 0;
        while (got[at] == (unsigned char)want[at])
            at++;
        FAIL("%s %d x %d: the texts differ from byte %zu of %zu", k_family[family], width, rows, at, want_bytes);
    }
    for (unsigned long long i = 0; i < bound + 64; i++)
        if (stores[i] != (i < length ? 1 : 0))
        {
            FAIL("%s %d x %d: byte %llu of %llu stored %d times", k_family[family], width, rows, i, length, stores[i]);
            break;
        }
    if (length > bound)
        FAIL("%s %d x %d: %llu bytes, the bound is %llu", k_family[family], width, rows, length, bound);
    if ((family == NOTHING || family == SAME_INDEX) && length != 0)
        FAIL("%s %d x %d: %llu bytes", k_family[family], width, rows, length);
    if (family == SAME_INDEX)
    { /* the 24-bit text of the same pair: every cell changed, all neighbours different */
        const unsigned long long most = KIND_RGB_MOST(width, rows);
        char *rgb_text = (char *)malloc((size_t)KIND_RGB_BOUND(width, rows));
        size_t rgb_bytes = 0;
        if (KIND_RGB_EMITTER(shown, next, width, rows, rgb_text, (size_t)KIND_RGB_BOUND(width, rows), &rgb_bytes) != TRT_HOST_OK || rgb_bytes != most)
            FAIL("same index %d x %d: the 24-bit delta text has %zu bytes, its longest has %llu", width, rows, rgb_bytes, most);
        free(rgb_text);
    }
    kind_verdicts(family, width, rows, length, bound, shown, next);
    free(shown), free(next), free(want), free(got), free(stores), free(tile_bytes), free(tile_at);
    return length;
}

/* bits of k_lengths that the family is there to make */
static void must_have_seen(int family, unsigned bits)
{
    if ((g_seen[family] & bits) != bits)
        FAIL("%s: record lengths seen %#x, wanted %#x", k_family[family], g_seen[family], bits);
}

/* The bound, by enumeration: every pattern of changed cells of a row of `width` cells with every pattern of "as the left neighbour", a cell at
 * a time; kind_cell_bytes(changed_left, state, changed_right) is the header's length of a record, `state` 0 an unchanged cell and 1 ..
 * KIND_STATES - 1 the changed cell's equalities with its left neighbour.  *longest: the longest row seen. */
static void enumerate_row(int width, int at, int before, int state, unsigned long long sum, unsigned long long *longest, unsigned long long *patterns)
{ /* `state` is cell at - 1's, `before` whether cell at - 2 changed; cell at - 1's record is known once cell `at` is chosen */
    if (at == width)
    {
        if (at > 0)
            sum += kind_cell_bytes(before, state, 0);
        if (sum > *longest)
            *longest = sum;
        ++*patterns;
        return;
    }
    for (int s = 0; s < KIND_STATES; s++)
        enumerate_row(width, at + 1, state != 0, s, at > 0 ? sum + kind_cell_bytes(before, state, s != 0) : sum, longest, patterns);
}

static void check_bound_by_enumeration(void)
{
    for (int width = 1; width <= 12; width++)
    {
        unsigned long long longest = 0, patterns = 0;
        enumerate_row(width, 0, 0, 0, 0, &longest, &patterns);
        if (longest != KIND_ROW_BOUND(width))
            FAIL("width %d: the longest of %llu rows has %llu bytes, the bound is %llu", width, patterns, longest, KIND_ROW_BOUND(width));
    }
}

static int verdict(void)
{
    if (g_failures)
    {
        fprintf(stderr, CHECK_NAME ": %d failure(s)\n", g_failures);
        return 1;
    }
    printf(CHECK_NAME ": ok (%ld cases)\n", g_cases);
    return 0;
}
