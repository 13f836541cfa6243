/* ansi_delta_check.h -- what the two check programs of the delta texts share (ansi_delta_check.c: the full text's cells; ansi_delta_half_check.c:
 * half-block cells): the generator, the families of frame pairs, and check(), which assembles a pair's text THROUGH THE KERNELS' OWN WALK and
 * holds it against the sequential emitter.  A program defines its kind and includes this file once:
 *
 *   CHECK_NAME            its name, for its messages
 *   KIND_LANE             the header's lane type                      trt_delta_lane            trt_delta_half_lane
 *   KIND_LANE_CELLS       the lane's walk                             trt_delta_lane_cells      trt_delta_half_lane_cells
 *   KIND_LANE_BYTE        byte k of the lane's j-th record            trt_delta_lane_byte       trt_delta_half_lane_byte
 *   KIND_EMITTER          the sequential statement (trt_emit.c)       trt_emitter_delta_rgb8    trt_emitter_delta_half_rgb8
 *   KIND_BOUND            the most bytes of a text
 *   KIND_TEXT_ROWS(rows)  rows of cells of a frame of `rows` pixel rows
 *   KIND_RECORD_MAX       the longest record
 *   k_lengths[], LENGTHS  every length a record can have
 *   kind_verdicts()       what the kind says of a family's length
 *
 * check() goes about it as the device does (csrc/trt_ansi_delta.hpp): for every tile and every thread 0 .. TRT_DELTA_BLOCK - 1 it calls
 * KIND_LANE_CELLS -- the function the kernels call with (blockIdx.x, threadIdx.x), which decides which bytes of the two frames are loaded -- and
 * sums the lanes' totals per tile (measure); scans the tiles' sums exclusively in turns of TRT_DELTA_SCAN_BLOCK with a running total (offsets);
 * and places each lane at its tile's offset plus the totals of the lanes before it, its records' bytes by KIND_LANE_BYTE (write), into a buffer
 * with a count per byte.  The frames are allocated at exactly rows * width * 3 bytes: a load behind a frame is the address sanitizer's to report.
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

/* the first SHARED_FAMILIES are both kinds'; those behind them make the record lengths that only half-block cells have */
enum
{
    NOTHING,       /* nothing changed */
    ALL_DIFFERENT, /* every pixel changed, all horizontal neighbours different: the bound (of half-block cells: an even frame's) */
    ALL_ONE,       /* every pixel changed, one colour (half-block: both colours equal the left neighbour's, the 3- and 7-byte records) */
    ALTERNATE,     /* every other pixel */
    FIRST_ONLY,
    LAST_ONLY,
    ACROSS_ROWS,   /* a run into a pixel row's last cell, one from the next row's first cell, the same colour */
    LEFT_COLOUR,   /* a changed pixel whose new colour is its unchanged left neighbour's */
    RANDOM_TWO_001, RANDOM_TWO_40, RANDOM_TWO_99, RANDOM_FULL_001, RANDOM_FULL_40, RANDOM_FULL_99,
    SHARED_FAMILIES,
    UPPER_ONLY = SHARED_FAMILIES, /* only the cells' upper pixel rows changed */
    LOWER_ONLY,                   /* only the lower ones */
    SAME_UPPER,                   /* every cell changed, the upper colour equals the left neighbour's while the lower differs: 22 and 26 bytes */
    SAME_LOWER,                   /* the converse */
    ALL_FAMILIES
};
static const char *const k_family[ALL_FAMILIES] = {"nothing", "all different", "all one colour", "alternate", "first only", "last only", "across rows", "left colour",
                                                   "random two 0.01", "random two 0.4", "random two 0.99", "random full 0.01", "random full 0.4", "random full 0.99",
                                                   "upper only", "lower only", "same upper", "same lower"};
static unsigned g_seen[ALL_FAMILIES]; /* bit i: a record of k_lengths[i] bytes occurred */

static void kind_verdicts(int family, int width, int rows, unsigned long long length, unsigned long long bound, const unsigned char *shown, const unsigned char *next);

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

/* pixel row r: every pixel another colour than it was and than its new left neighbour */
static void row_all_different(const unsigned char *shown, unsigned char *next, int width, int r)
{
    for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
        put(next, p, other_than(get(shown, p), p % width ? get(next, p - 1) : get(shown, p)));
}
/* pixel row r: every pixel changed, to one colour */
static void row_all_one(unsigned char *shown, unsigned char *next, int width, int r)
{
    for (long long p = (long long)r * width; p < (long long)(r + 1) * width; p++)
        put(shown, p, 0x102030u + (unsigned)(p & 1)), put(next, p, 0xa0b0c0u);
}

static void make_frames(int family, int width, int rows, unsigned char *shown, unsigned char *next)
{
    const long long pixels = (long long)width * rows;
    for (long long p = 0; p < pixels; p++)
        put(shown, p, next_random() & 0xffffffu);
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

static void check(int family, int width, int rows)
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
    if (family == NOTHING && length != 0)
        FAIL("nothing changed %d x %d: %llu bytes", width, rows, length);
    kind_verdicts(family, width, rows, length, bound, shown, next);
    free(shown), free(next), free(want), free(got), free(stores), free(tile_bytes), free(tile_at);
}

/* bits of k_lengths that the family is there to make */
static void must_have_seen(int family, unsigned bits)
{
    if ((g_seen[family] & bits) != bits)
        FAIL("%s: record lengths seen %#x, wanted %#x", k_family[family], g_seen[family], bits);
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
