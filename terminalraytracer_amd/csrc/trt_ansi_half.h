/*
 * trt_ansi_half.h -- the layout of a frame's HALF-BLOCK terminal text (host + device, plain C).
 *
 * The text of trt_ansi.h paints a pixel as two spaces on a background colour: two columns and a whole line.  This one paints TWO
 * pixels per character cell with the upper-half-block glyph U+2580: the foreground colour fills the upper half of the cell, the
 * background colour the lower half, so one column and half a line make a (square) pixel.  The reference has no such emitter; the
 * format is the project's own.  For a screen of `width` x `rows` owned rows, T = (rows + 1) / 2 text rows, in order,
 *
 *      "\033[0;0H"                                                              6 bytes, the home prefix (reset_str, TRT.c:1102)
 *      per text row i:  width cells "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm" E2 96 80     39 bytes each
 *                       "\033[0m\n"                                             5 bytes
 *
 * RRR;GGG;BBB are the emitter's bytes of owned row 2 i (the upper pixel), rrr;ggg;bbb those of owned row 2 i + 1 (the lower pixel;
 * 000;000;000 behind the last row of an odd frame), three zero-padded digits each as byte_to_digits makes them (TRT.c:1134-1139).
 * No NUL follows: 6 + (39 width + 5) T bytes.  trt_emitter_half_rgb8 (csrc/host/trt_emit.c) is the sequential statement; this header
 * maps a position of the text to what stands there -- the device pass (trt_ansi_half.hpp) and the host check
 * (tests/ansi_half_check.c) compile the same map -- and says which lane of which wave stores which bytes.
 *
 * A position is a trt_ansi_half_at.  trt_ansi_half_locate finds it from nothing, with a 64-bit division by the row length: once per
 * WAVE on the device.  trt_ansi_half_advance finds the position d < TRT_ANSI_HALF_SPAN bytes behind a located one with 32-bit
 * arithmetic only (the row length divides by a compare or by a multiply-high with trt_ansi_half_row_magic, the cell length is a
 * constant), once per WORD; trt_ansi_half_step walks to the next byte.  A row's five end bytes count to its last cell.
 *
 * The lane map.  The text is stored as aligned 32-bit words: `head` = (-address) mod 4 bytes in front of the first aligned address,
 * then `words` words, then `tail` < 4 bytes.  The head lies in the home prefix (3 < 6) and the tail in the last row's end bytes
 * (3 < 5), so neither needs a pixel: wave 0's lanes 0..2 and 4..6 store them, a byte each (trt_ansi_half_lone_byte).  Wave g owns the
 * words [g, g + 1) * TRT_ANSI_HALF_WAVE_WORDS, lane l of it the words g * TRT_ANSI_HALF_WAVE_WORDS + 64 j + l, j = 0..8: every store
 * instruction of a wave covers 256 consecutive bytes.
 *
 * The bound.  A span of S bytes touches the most cells when it begins in a cell's last byte: that cell, and one more for every 39
 * bytes or part of them that follow -- (38 + S - 1) / 39 + 1 cells (end bytes and the prefix only make it fewer).  For the 2304
 * bytes of nine words per lane that is 61 <= 64 (TRT_ANSI_HALF_SPAN_CELLS): lane l holds cell C0 + l, C0 the cell of the wave's first
 * byte, and 61 of 64 lanes have two pixels to sum.  (Six words per lane, as the full text has, would leave a third of the lanes
 * without a cell.)
 *
 * Which colour a word needs.  A cell is longer than a word, so a word shows at most two cells.  The digits of a cell stand at 7..17
 * (upper pixel) and 24..34 (lower pixel): bytes 35..43 of a cell and bytes 0..6 of the next hold none, so a word that leaves its
 * first byte's cell shows no digit of either, and the upper and lower digits of one cell are 6 bytes apart, more than a word is
 * long.  Every digit of a word therefore belongs to the cell of its FIRST byte: a word is formatted from that one cell's two
 * colours.
 */
#ifndef TRT_ANSI_HALF_H
#define TRT_ANSI_HALF_H

#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_ANSI_HALF_HD __host__ __device__ __forceinline__
#else
#define TRT_ANSI_HALF_HD static inline
#endif

#define TRT_ANSI_HALF_HOME 6  /* strlen("\033[0;0H") */
#define TRT_ANSI_HALF_CELL 39 /* strlen("\033[38;2;000;000;000;48;2;000;000;000m") + the glyph's three bytes */
#define TRT_ANSI_HALF_END 5   /* strlen("\033[0m\n") */
#define TRT_ANSI_HALF_WAVE_WORDS 576 /* 9 words per lane */
#define TRT_ANSI_HALF_SPAN (4 * TRT_ANSI_HALF_WAVE_WORDS)
#define TRT_ANSI_HALF_SPAN_CELLS ((TRT_ANSI_HALF_CELL - 1 + TRT_ANSI_HALF_SPAN - 1) / TRT_ANSI_HALF_CELL + 1) /* 61: a wave's cells fit its lanes */

#define TRT_ANSI_HALF_PACK8(a, b, c, d, e, f, g, h)                                                                             \
    ((unsigned long long)(a) | (unsigned long long)(b) << 8 | (unsigned long long)(c) << 16 | (unsigned long long)(d) << 24 |   \
     (unsigned long long)(e) << 32 | (unsigned long long)(f) << 40 | (unsigned long long)(g) << 48 | (unsigned long long)(h) << 56)

typedef struct
{
    long long trow; /* text row; T = (rows + 1) / 2: behind the text (a word no lane stores) */
    long long r;    /* byte of the row's 39 width + 5; r < 0: byte r + 6 of the home prefix (text row 0) */
    int col;        /* cell of the row (0 in the prefix) */
    int c;          /* byte of the cell; 39..43: the row's end bytes, which count to its last cell */
} trt_ansi_half_at;

TRT_ANSI_HALF_HD long long trt_ansi_half_text_rows(long long rows) { return (rows + 1) / 2; }

TRT_ANSI_HALF_HD long long trt_ansi_half_row_bytes(int width) { return (long long)TRT_ANSI_HALF_CELL * width + TRT_ANSI_HALF_END; }

/* length of the text; 0 for a screen that has none */
TRT_ANSI_HALF_HD unsigned long long trt_ansi_half_text_bytes(int width, long long rows)
{
    if (width <= 0 || rows <= 0)
        return 0;
    return (unsigned long long)TRT_ANSI_HALF_HOME + (unsigned long long)trt_ansi_half_row_bytes(width) * (unsigned long long)trt_ansi_half_text_rows(rows);
}

/* min(ceil(2^32 / d), 2^32 - 1): x / d by multiply-high, exact while x * d < 2^32 */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_magic(unsigned long long d)
{
    const unsigned long long m = (0x100000000ull + d - 1) / d;
    return m > 0xffffffffull ? 0xffffffffu : (unsigned)m;
}

/* for the row length (trt_ansi_half_advance: x < 2 * 2304 where it is used) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_row_magic(int width) { return trt_ansi_half_magic((unsigned long long)trt_ansi_half_row_bytes(width)); }

/* for the width (trt_ansi_half_lane_cell: x < 128 where it is used) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_width_magic(int width) { return trt_ansi_half_magic((unsigned long long)width); }

/* the cell the position belongs to, counted through the text: 0 in the prefix */
TRT_ANSI_HALF_HD long long trt_ansi_half_cell(const trt_ansi_half_at *at, int width) { return at->trow * width + at->col; }

TRT_ANSI_HALF_HD trt_ansi_half_at trt_ansi_half_locate(unsigned long long position, int width, long long rows)
{
    const long long u = (long long)position - TRT_ANSI_HALF_HOME, row_bytes = trt_ansi_half_row_bytes(width), trows = trt_ansi_half_text_rows(rows);
    trt_ansi_half_at at = {0, u, 0, 0};
    if (u < 0)
        return at;
    at.trow = u / row_bytes;
    if (at.trow >= trows)
    {
        at.r = u - trows * row_bytes;
        at.trow = trows;
        return at;
    }
    at.r = u - at.trow * row_bytes;
    at.col = (int)(at.r / TRT_ANSI_HALF_CELL);
    if (at.col >= width)
        at.col = width - 1;
    at.c = (int)(at.r - (long long)at.col * TRT_ANSI_HALF_CELL);
    return at;
}

/* the position d < TRT_ANSI_HALF_SPAN bytes behind *from, which trt_ansi_half_locate found */
TRT_ANSI_HALF_HD trt_ansi_half_at trt_ansi_half_advance(const trt_ansi_half_at *from, unsigned d, int width, long long rows, unsigned row_magic)
{
    const long long row_bytes = trt_ansi_half_row_bytes(width), trows = trt_ansi_half_text_rows(rows), x = from->r + (long long)d;
    trt_ansi_half_at at = {from->trow, x, 0, 0};
    if (x < 0 || from->trow >= trows) /* still in the prefix; behind the text */
        return at;
    /* x < row bytes + 2304: no or one row further on where rows are long, and a 32-bit quotient where they are short */
    const unsigned q = row_bytes >= TRT_ANSI_HALF_SPAN ? (unsigned)(x >= row_bytes) : (unsigned)(((unsigned long long)(unsigned)x * row_magic) >> 32);
    at.trow = from->trow + q;
    at.r = x - (long long)q * row_bytes;
    if (at.trow >= trows)
    {
        at.r = x - (trows - from->trow) * row_bytes;
        at.trow = trows;
        return at;
    }
    /* in from's row, counted from from's cell: < 44 + 2304; in a later row r itself is < 2304 */
    const int base = q == 0 ? from->col : 0;
    const unsigned e = (unsigned)(at.r - (long long)base * TRT_ANSI_HALF_CELL), cells = e / TRT_ANSI_HALF_CELL;
    at.col = base + (int)cells;
    at.c = (int)(e - cells * TRT_ANSI_HALF_CELL);
    if (at.col >= width) /* the end bytes: at most 43 behind the last cell's first byte, so one cell too far at the most */
        at.col = width - 1, at.c += TRT_ANSI_HALF_CELL;
    return at;
}

/* to the next byte; 1 when it belongs to another cell than the one left.  Selects, no branches: 64 lanes walk different bytes */
TRT_ANSI_HALF_HD int trt_ansi_half_step(trt_ansi_half_at *at, int width, long long rows)
{
    const long long r = at->r + 1;
    const int inside = r > 0 && at->trow < trt_ansi_half_text_rows(rows); /* r == 0: from the prefix into cell 0 of row 0, which is where col and c already are */
    const int c = at->c + inside;
    const int next_cell = inside & (c == TRT_ANSI_HALF_CELL) & (at->col + 1 < width), next_row = inside & (c >= TRT_ANSI_HALF_CELL + TRT_ANSI_HALF_END);
    at->col = next_row ? 0 : at->col + next_cell;
    at->c = next_cell | next_row ? 0 : c;
    at->trow += next_row;
    at->r = next_row ? 0 : r;
    return next_cell | next_row;
}

/* byte c < 44 of a cell (39..43: the end bytes behind a row's last cell) whose upper pixel is upper = r | g << 8 | b << 16 and whose
 * lower pixel is lower */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_cell_byte(int c, unsigned upper, unsigned lower)
{
    const unsigned long long k0 = TRT_ANSI_HALF_PACK8(0x1b, '[', '3', '8', ';', '2', ';', '0'), k1 = TRT_ANSI_HALF_PACK8('0', '0', ';', '0', '0', '0', ';', '0'),
                             k2 = TRT_ANSI_HALF_PACK8('0', '0', ';', '4', '8', ';', '2', ';'), k3 = TRT_ANSI_HALF_PACK8('0', '0', '0', ';', '0', '0', '0', ';'),
                             k4 = TRT_ANSI_HALF_PACK8('0', '0', '0', 'm', 0xe2, 0x96, 0x80, 0x1b), k5 = TRT_ANSI_HALF_PACK8('[', '0', 'm', '\n', 0, 0, 0, 0);
    const unsigned long long k = c < 8 ? k0 : c < 16 ? k1 : c < 24 ? k2 : c < 32 ? k3 : c < 40 ? k4 : k5;
    const int low = c >= 24;                        /* digits at 7..9, 11..13, 15..17 and at 24..26, 28..30, 32..34 */
    const unsigned d = (unsigned)(c - (low ? 24 : 7)), rgb = low ? lower : upper;
    const unsigned v = (rgb >> (((d >> 2) & 3u) * 8)) & 0xffu, place = d & 3u;
    const unsigned digit = place == 0 ? v / 100u : place == 1 ? (v / 10u) % 10u : v % 10u;
    return ((unsigned)(k >> ((c & 7) * 8)) & 0xffu) + (d < 11u && place != 3u ? digit : 0u);
}

/* what stands at *at inside the text, upper and lower being the pixels of trt_ansi_half_cell(at) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_byte(const trt_ansi_half_at *at, unsigned upper, unsigned lower)
{
    const unsigned home = (unsigned)(TRT_ANSI_HALF_PACK8(0x1b, '[', '0', ';', '0', 'H', 0, 0) >> (((at->r + TRT_ANSI_HALF_HOME) & 7) * 8)) & 0xffu;
    return at->r < 0 ? home : trt_ansi_half_cell_byte(at->c & 63, upper, lower);
}

/* ---- who stores what ---- */

typedef struct
{
    unsigned head, tail;      /* bytes in front of the first 4-aligned address of the text, bytes behind the last word */
    unsigned long long words; /* aligned 32-bit words between them */
} trt_ansi_half_split;

TRT_ANSI_HALF_HD trt_ansi_half_split trt_ansi_half_split_of(unsigned long long address, unsigned long long bytes)
{
    trt_ansi_half_split s;
    s.head = (unsigned)((4 - (address & 3)) & 3);
    if (s.head > bytes)
        s.head = (unsigned)bytes;
    s.words = (bytes - s.head) / 4;
    s.tail = (unsigned)((bytes - s.head) % 4);
    return s;
}

/* waves of a text of `words` words: wave 0 is there for the lone bytes however short the text */
TRT_ANSI_HALF_HD unsigned long long trt_ansi_half_waves(unsigned long long words)
{
    const unsigned long long waves = (words + TRT_ANSI_HALF_WAVE_WORDS - 1) / TRT_ANSI_HALF_WAVE_WORDS;
    return waves ? waves : 1;
}

/* the word lane `lane` of wave `wave` stores in its turn j < 9; the wave's words are those below `words` */
TRT_ANSI_HALF_HD unsigned long long trt_ansi_half_lane_word(unsigned long long wave, int lane, int j)
{
    return wave * TRT_ANSI_HALF_WAVE_WORDS + (unsigned)(64 * j + lane);
}

/* The cell lane `lane` < 64 holds in a wave whose first byte is at *from: text row and column of cell trt_ansi_half_cell(from) + lane.
 * from->col + lane < width + 64: no or one row further on where rows are wide, a multiply-high where they are narrow (x < 128; the
 * magic of width 1 would be 2^32, which 32 bits do not hold: there the quotient is x itself). */
TRT_ANSI_HALF_HD void trt_ansi_half_lane_cell(const trt_ansi_half_at *from, int lane, int width, unsigned width_magic, long long *trow, int *col)
{
    const unsigned x = (unsigned)from->col + (unsigned)lane;
    const unsigned q = width >= 64 ? (unsigned)(x >= (unsigned)width) : width == 1 ? x : (unsigned)(((unsigned long long)x * width_magic) >> 32);
    *trow = from->trow + q;
    *col = (int)(x - q * (unsigned)width);
}

/* the position of the byte that lane `lane` of wave 0 stores by itself, or -1: the head's bytes, lanes 0..2, and the tail's, lanes 4..6 */
TRT_ANSI_HALF_HD long long trt_ansi_half_lone_byte(const trt_ansi_half_split *s, int lane)
{
    if (lane < (int)s->head)
        return lane;
    if (lane >= 4 && lane - 4 < (int)s->tail)
        return (long long)(s->head + 4 * s->words) + (lane - 4);
    return -1;
}

/* ... and its value in a text of `bytes` bytes: the head is in the home prefix, the tail in the last row's end bytes (a text is at
 * least 50 bytes long) */
TRT_ANSI_HALF_HD unsigned trt_ansi_half_lone_value(long long position, unsigned long long bytes)
{
    const trt_ansi_half_at at = {0, position - TRT_ANSI_HALF_HOME, 0, 0};
    return position < TRT_ANSI_HALF_HOME ? trt_ansi_half_byte(&at, 0, 0)
                                         : trt_ansi_half_cell_byte(TRT_ANSI_HALF_CELL + TRT_ANSI_HALF_END - (int)((long long)bytes - position), 0, 0);
}

#endif /* TRT_ANSI_HALF_H */
