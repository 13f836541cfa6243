/*
 * trt_ansi.h -- the layout of a frame's terminal text (host + device, plain C).
 *
 * buffered_draw_screen (TRT.c:1142-1172) patches nine decimal digits per pixel into a pre-formatted buffer and writes all of it:
 * for a frame of `width` x `rows` owned rows, in order,
 *
 *      "\033[0;0H"                                               6 bytes, the home prefix
 *      per row:  width cells "\033[48;2;RRR;GGG;BBBm  \033[0m"  25 bytes each, then '\n'
 *      three NUL bytes                                           (the reference writes sizeof(screenbuffer), TRT.c:1104)
 *
 * 8 + (25 width + 1) rows + 1 bytes: what trt_emitter_create / trt_emitter_patch_rgb8 (csrc/host/trt_emit.c) leave in the emitter's
 * buffer.  This header maps a position of the text to what stands there -- the device pass that writes the text (trt_ansi.hpp) and
 * the host check (tests/ansi_check.c) compile the same map -- and says which lane of which wave stores which bytes.
 *
 * A position is a trt_ansi_at.  trt_ansi_locate finds it from nothing, with a 64-bit division by the row length: once per WAVE on
 * the device.  trt_ansi_advance finds the position d < TRT_ANSI_SPAN bytes behind a located one with 32-bit arithmetic only (the row
 * length divides by a compare or by a multiply-high with trt_ansi_row_magic, the cell length is a constant), once per WORD;
 * trt_ansi_step walks to the next byte.
 *
 * The lane map.  The text is stored as aligned 32-bit words: `head` = (-address) mod 4 bytes in front of the first aligned address,
 * then `words` words, then `tail` < 4 bytes.  The head lies in the home prefix (3 < 6) and the tail in the three NULs, so neither
 * needs a pixel: wave 0's lanes 0..2 and 4..6 store them, a byte each (trt_ansi_lone_byte).  Wave g owns the words
 * [g, g + 1) * TRT_ANSI_WAVE_WORDS, lane l of it the words g * TRT_ANSI_WAVE_WORDS + 64 j + l, j = 0..5: every store instruction of a
 * wave covers 256 consecutive bytes.  A span of 1536 bytes that begins c bytes into a cell ends at most (24 + 1535) / 25 = 62 cells
 * further on: the pixels a wave's words show are P0 .. P0 + 62, P0 the pixel of the wave's first byte, and lane l holds pixel P0 + l.
 */
#ifndef TRT_ANSI_H
#define TRT_ANSI_H

#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_ANSI_HD __host__ __device__ __forceinline__
#else
#define TRT_ANSI_HD static inline
#endif

#define TRT_ANSI_HOME 6 /* strlen("\033[0;0H"), reset_str of TRT.c:1102 */
#define TRT_ANSI_CELL 25 /* strlen(pixel_str), TRT.c:1103 */
#define TRT_ANSI_NULS 3
#define TRT_ANSI_WAVE_WORDS 384 /* 6 words per lane */
#define TRT_ANSI_SPAN (4 * TRT_ANSI_WAVE_WORDS)

#define TRT_ANSI_PACK8(a, b, c, d, e, f, g, h)                                                                                  \
    ((unsigned long long)(a) | (unsigned long long)(b) << 8 | (unsigned long long)(c) << 16 | (unsigned long long)(d) << 24 |   \
     (unsigned long long)(e) << 32 | (unsigned long long)(f) << 40 | (unsigned long long)(g) << 48 | (unsigned long long)(h) << 56)

typedef struct
{
    long long row; /* owned row; `rows`: behind the last row, in the three NULs */
    long long r;   /* byte of the row's 25 width + 1; r < 0: byte r + 6 of the home prefix (row 0); behind the last row: byte of the NULs */
    int col;       /* cell of the row (0 in the prefix and in the NULs) */
    int c;         /* byte of the cell; 25: the newline, which counts to its row's last cell */
} trt_ansi_at;

TRT_ANSI_HD long long trt_ansi_row_bytes(int width) { return (long long)TRT_ANSI_CELL * width + 1; }

/* length of the text; 0 for a screen that has none */
TRT_ANSI_HD unsigned long long trt_ansi_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0)
        return 0;
    return (unsigned long long)(TRT_ANSI_HOME + 2) + (unsigned long long)trt_ansi_row_bytes(width) * (unsigned long long)rows + 1;
}

/* min(ceil(2^32 / row bytes), 2^32 - 1): x / row bytes by multiply-high, exact while x * row bytes < 2^32 (trt_ansi_advance: x < 2 * 1536) */
TRT_ANSI_HD unsigned trt_ansi_row_magic(int width)
{
    const unsigned long long d = (unsigned long long)trt_ansi_row_bytes(width), m = (0x100000000ull + d - 1) / d;
    return m > 0xffffffffull ? 0xffffffffu : (unsigned)m;
}

/* the pixel whose cell the position belongs to: 0 in the prefix, width * rows in the NULs */
TRT_ANSI_HD long long trt_ansi_pixel(const trt_ansi_at *at, int width) { return at->row * width + at->col; }

TRT_ANSI_HD trt_ansi_at trt_ansi_locate(unsigned long long position, int width, long long rows)
{
    const long long u = (long long)position - TRT_ANSI_HOME, row_bytes = trt_ansi_row_bytes(width);
    trt_ansi_at at = {0, u, 0, 0};
    if (u < 0)
        return at;
    at.row = u / row_bytes;
    if (at.row >= rows)
    {
        at.r = u - rows * row_bytes;
        at.row = rows;
        return at;
    }
    at.r = u - at.row * row_bytes;
    at.col = (int)(at.r / TRT_ANSI_CELL);
    at.c = (int)(at.r - (long long)at.col * TRT_ANSI_CELL);
    if (at.col == width)
        at.col = width - 1, at.c = TRT_ANSI_CELL;
    return at;
}

/* the position d < TRT_ANSI_SPAN bytes behind *from, which trt_ansi_locate found */
TRT_ANSI_HD trt_ansi_at trt_ansi_advance(const trt_ansi_at *from, unsigned d, int width, long long rows, unsigned row_magic)
{
    const long long row_bytes = trt_ansi_row_bytes(width), x = from->r + (long long)d;
    trt_ansi_at at = {from->row, x, 0, 0};
    if (x < 0 || from->row >= rows) /* still in the prefix; in the NULs */
        return at;
    /* x < row bytes + 1536: no or one row further on where rows are long, and a 32-bit quotient where they are short */
    const unsigned q = row_bytes >= TRT_ANSI_SPAN ? (unsigned)(x >= row_bytes)
                                                  : (unsigned)(((unsigned long long)(unsigned)x * row_magic) >> 32);
    at.row = from->row + q;
    at.r = x - (long long)q * row_bytes;
    if (at.row >= rows)
    {
        at.r = x - (rows - from->row) * row_bytes;
        at.row = rows;
        return at;
    }
    /* in from's row, counted from from's cell: < 25 + 1536; in a later row r itself is < 1536 */
    const int base = q == 0 ? from->col : 0;
    const unsigned e = (unsigned)(at.r - (long long)base * TRT_ANSI_CELL), cells = e / TRT_ANSI_CELL;
    at.col = base + (int)cells;
    at.c = (int)(e - cells * TRT_ANSI_CELL);
    if (at.col == width)
        at.col = width - 1, at.c = TRT_ANSI_CELL;
    return at;
}

/* to the next byte; 1 when it belongs to another pixel than the one left.  Selects, no branches: 64 lanes walk different bytes */
TRT_ANSI_HD int trt_ansi_step(trt_ansi_at *at, int width, long long rows)
{
    const long long r = at->r + 1;
    const int inside = r > 0 && at->row < rows; /* r == 0: from the prefix into cell 0 of row 0, which is where col and c already are */
    const int c = at->c + inside;
    const int next_cell = inside & (c == TRT_ANSI_CELL) & (at->col + 1 < width), next_row = inside & (c > TRT_ANSI_CELL);
    at->col = next_row ? 0 : at->col + next_cell;
    at->c = next_cell | next_row ? 0 : c;
    at->row += next_row;
    at->r = next_row ? 0 : r;
    return next_cell | next_row;
}

/* byte c of the cell of a pixel rgb = r | g << 8 | b << 16: pixel_str with byte_to_digits' digits in it (TRT.c:1134-1139) */
TRT_ANSI_HD unsigned trt_ansi_cell_byte(int c, unsigned rgb)
{
    const unsigned long long k0 = TRT_ANSI_PACK8(0x1b, '[', '4', '8', ';', '2', ';', '0'), k1 = TRT_ANSI_PACK8('0', '0', ';', '0', '0', '0', ';', '0'),
                             k2 = TRT_ANSI_PACK8('0', '0', 'm', ' ', ' ', 0x1b, '[', '0'), k3 = 'm';
    const unsigned long long k = c < 8 ? k0 : c < 16 ? k1 : c < 24 ? k2 : k3;
    const unsigned d = (unsigned)(c - 7); /* digits at 7..9, 11..13, 15..17 */
    const unsigned v = (rgb >> (((d >> 2) & 3u) * 8)) & 0xffu, place = d & 3u;
    const unsigned digit = place == 0 ? v / 100u : place == 1 ? (v / 10u) % 10u : v % 10u;
    return ((unsigned)(k >> ((c & 7) * 8)) & 0xffu) + (d < 11u && place != 3u ? digit : 0u);
}

/* what stands at *at, rgb being the bytes of trt_ansi_pixel(at) */
TRT_ANSI_HD unsigned trt_ansi_byte(const trt_ansi_at *at, long long rows, unsigned rgb)
{
    const unsigned home = (unsigned)(TRT_ANSI_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0) >> (((at->r + TRT_ANSI_HOME) & 7) * 8)) & 0xffu;
    const unsigned cell = at->c == TRT_ANSI_CELL ? (unsigned)'\n' : trt_ansi_cell_byte(at->c & 31, rgb);
    return at->r < 0 ? home : at->row >= rows ? 0u : cell;
}

/* ---- who stores what ---- */

typedef struct
{
    unsigned head, tail;      /* bytes in front of the first 4-aligned address of the text, bytes behind the last word */
    unsigned long long words; /* aligned 32-bit words between them */
} trt_ansi_split;

TRT_ANSI_HD trt_ansi_split trt_ansi_split_of(unsigned long long address, unsigned long long bytes)
{
    trt_ansi_split s;
    s.head = (unsigned)((4 - (address & 3)) & 3);
    if (s.head > bytes)
        s.head = (unsigned)bytes;
    s.words = (bytes - s.head) / 4;
    s.tail = (unsigned)((bytes - s.head) % 4);
    return s;
}

/* waves of a text of `words` words: wave 0 is there for the lone bytes however short the text */
TRT_ANSI_HD unsigned long long trt_ansi_waves(unsigned long long words)
{
    const unsigned long long waves = (words + TRT_ANSI_WAVE_WORDS - 1) / TRT_ANSI_WAVE_WORDS;
    return waves ? waves : 1;
}

/* the word lane `lane` of wave `wave` stores in its turn j < 6; the wave's words are those below `words` */
TRT_ANSI_HD unsigned long long trt_ansi_lane_word(unsigned long long wave, int lane, int j)
{
    return wave * TRT_ANSI_WAVE_WORDS + (unsigned)(64 * j + lane);
}

/* the position of the byte that lane `lane` of wave 0 stores by itself, or -1: the head's bytes, lanes 0..2, and the tail's, lanes 4..6 */
TRT_ANSI_HD long long trt_ansi_lone_byte(const trt_ansi_split *s, int lane)
{
    if (lane < (int)s->head)
        return lane;
    if (lane >= 4 && lane - 4 < (int)s->tail)
        return (long long)(s->head + 4 * s->words) + (lane - 4);
    return -1;
}

/* ... and its value: the head is in the home prefix, the tail in the NULs (a text is at least 35 bytes long) */
TRT_ANSI_HD unsigned trt_ansi_lone_value(long long position)
{
    const trt_ansi_at at = {0, position - TRT_ANSI_HOME, 0, 0};
    return position < TRT_ANSI_HOME ? trt_ansi_byte(&at, 1, 0) : 0u;
}

#endif /* TRT_ANSI_H */
