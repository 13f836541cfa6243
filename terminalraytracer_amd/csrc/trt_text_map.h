/*
 * trt_text_map.h -- the position map and the lane map of a frame's WHOLE terminal text, for both formats (host + device, plain C).
 *
 * A whole text (trt_ansi.h: two spaces a pixel; trt_ansi_half.h: half-block cells, two pixel rows a line) is, in order,
 *
 *      "\033[0;0H"                                  6 bytes, the home prefix (reset_str, TRT.c:1102)
 *      per text row:  width cells of `cell` bytes, then `end` bytes that end the row
 *      `nuls` NUL bytes
 *
 * and a trt_text_kind holds those numbers and `wave_words`, the aligned 32-bit words a wave of the device pass stores.  A format header
 * makes its kind of LITERALS (trt_ansi_kind, trt_ansi_half_kind) and every function here is inlined into its caller, so that a division
 * by kind.cell is a division by a constant wherever it is compiled.  What stands in a cell, in the end bytes and in the prefix is the
 * format's own: its header maps a position found here to a byte.  The device pass (text_write, trt_ansi.hpp) and the host checks
 * (tests/ansi_text_check.h) compile the same functions.
 *
 * A position is a trt_text_at.  trt_text_locate finds it from nothing, with a 64-bit division by the row length: once per WAVE on the
 * device.  trt_text_advance finds the position d < span = 4 wave_words bytes behind a located one with 32-bit arithmetic only (the row
 * length divides by a compare or by a multiply-high with trt_text_magic of it, the cell length is a constant), once per WORD;
 * trt_text_step walks to the next byte.  A row's end bytes count to its last cell.
 *
 * The lane map.  The text is stored as aligned 32-bit words: `head` = (-address) mod 4 bytes in front of the first aligned address,
 * then `words` words, then `tail` < 4 bytes.  The head lies in the home prefix (3 < 6) and the tail in the text's last bytes -- the full
 * text's three NULs, the five end bytes of the half-block text's last row (3 < 5) -- so neither needs a pixel: wave 0's lanes 0..2 and
 * 4..6 store them, a byte each (trt_text_lone_byte; the value is the format's *_lone_value).  Wave g owns the words
 * [g, g + 1) * wave_words, lane l of it the words g * wave_words + 64 j + l, j < wave_words / 64: every store instruction of a wave
 * covers 256 consecutive bytes.
 *
 * The bound.  A span of S bytes touches the most cells when it begins in a cell's last byte: that cell, and one more for every `cell`
 * bytes or part of them that follow -- TRT_TEXT_SPAN_CELLS = (cell - 1 + S - 1) / cell + 1 cells (end bytes, the prefix and the NULs
 * only make it fewer).  Lane l of a wave holds cell C0 + l, C0 the cell of the wave's first byte, so the bound must not exceed 64:
 * the 1536 bytes of the full text's six words per lane touch 63 cells of 25 bytes (the pixels P0 .. P0 + 62), the 2304 bytes of the
 * half-block text's nine words per lane 61 cells of 39 (six words per lane would leave a third of the lanes without a cell).
 */
#ifndef TRT_TEXT_MAP_H
#define TRT_TEXT_MAP_H

#if defined(__HIPCC__) || defined(__HIP__)
#define TRT_TEXT_HD __host__ __device__ __forceinline__
#else
#define TRT_TEXT_HD static inline __attribute__((always_inline))
#endif

#define TRT_TEXT_HOME 6 /* strlen("\033[0;0H"), reset_str of TRT.c:1102 */
#define TRT_TEXT_SPAN_CELLS(cell, wave_words) (((cell)-1 + 4 * (wave_words)-1) / (cell) + 1)

#define TRT_TEXT_PACK8(a, b, c, d, e, f, g, h)                                                                                  \
    ((unsigned long long)(a) | (unsigned long long)(b) << 8 | (unsigned long long)(c) << 16 | (unsigned long long)(d) << 24 |   \
     (unsigned long long)(e) << 32 | (unsigned long long)(f) << 40 | (unsigned long long)(g) << 48 | (unsigned long long)(h) << 56)

typedef struct
{
    int cell;       /* bytes of a cell */
    int end;        /* bytes that end a text row, behind its last cell */
    int wave_words; /* aligned words a wave stores, a multiple of 64; its span is four times as many bytes */
    int nuls;       /* NUL bytes behind the last row */
} trt_text_kind;

typedef struct
{
    long long row; /* text row; `trows`, the text's rows: behind the last row */
    long long r;   /* byte of the row's cell width + end; r < 0: byte r + 6 of the home prefix (row 0); behind the last row: byte of what stands there */
    int col;       /* cell of the row (0 in the prefix and behind the last row) */
    int c;         /* byte of the cell; cell .. cell + end - 1: the row's end bytes, which count to its last cell */
} trt_text_at;

TRT_TEXT_HD long long trt_text_row_bytes(const trt_text_kind kind, int width) { return (long long)kind.cell * width + kind.end; }

/* min(ceil(2^32 / d), 2^32 - 1): x / d by multiply-high, exact while x * d < 2^32 (trt_text_advance: d the row length, x < 2 span) */
TRT_TEXT_HD unsigned trt_text_magic(unsigned long long d)
{
    const unsigned long long m = (0x100000000ull + d - 1) / d;
    return m > 0xffffffffull ? 0xffffffffu : (unsigned)m;
}

/* the cell the position belongs to, counted through the text: 0 in the prefix, width * trows behind the last row */
TRT_TEXT_HD long long trt_text_cell(const trt_text_at *at, int width) { return at->row * width + at->col; }

TRT_TEXT_HD trt_text_at trt_text_locate(const trt_text_kind kind, unsigned long long position, int width, long long trows)
{
    const long long u = (long long)position - TRT_TEXT_HOME, row_bytes = trt_text_row_bytes(kind, width);
    trt_text_at at = {0, u, 0, 0};
    if (u < 0)
        return at;
    at.row = u / row_bytes;
    if (at.row >= trows)
    {
        at.r = u - trows * row_bytes;
        at.row = trows;
        return at;
    }
    at.r = u - at.row * row_bytes;
    at.col = (int)(at.r / kind.cell);
    if (at.col >= width) /* the end bytes */
        at.col = width - 1;
    at.c = (int)(at.r - (long long)at.col * kind.cell);
    return at;
}

/* the position d < 4 kind.wave_words bytes behind *from, which trt_text_locate found */
TRT_TEXT_HD trt_text_at trt_text_advance(const trt_text_kind kind, const trt_text_at *from, unsigned d, int width, long long trows, unsigned row_magic)
{
    const long long row_bytes = trt_text_row_bytes(kind, width), x = from->r + (long long)d;
    trt_text_at at = {from->row, x, 0, 0};
    if (x < 0 || from->row >= trows) /* still in the prefix; behind the last row */
        return at;
    /* x < row bytes + span: no or one row further on where rows are long, and a 32-bit quotient where they are short */
    const unsigned q = row_bytes >= 4 * kind.wave_words ? (unsigned)(x >= row_bytes) : (unsigned)(((unsigned long long)(unsigned)x * row_magic) >> 32);
    at.row = from->row + q;
    at.r = x - (long long)q * row_bytes;
    if (at.row >= trows)
    {
        at.r = x - (trows - from->row) * row_bytes;
        at.row = trows;
        return at;
    }
    /* in from's row, counted from from's cell: < cell + end + span; in a later row r itself is < span */
    const int base = q == 0 ? from->col : 0;
    const unsigned e = (unsigned)(at.r - (long long)base * kind.cell), cells = e / (unsigned)kind.cell;
    at.col = base + (int)cells;
    at.c = (int)(e - cells * (unsigned)kind.cell);
    if (at.col >= width) /* the end bytes: less than cell + end behind the last cell's first byte, so one cell too far at the most (end <= cell) */
        at.col = width - 1, at.c += kind.cell;
    return at;
}

/* to the next byte; 1 when it belongs to another cell than the one left.  Selects, no branches: 64 lanes walk different bytes */
TRT_TEXT_HD int trt_text_step(const trt_text_kind kind, trt_text_at *at, int width, long long trows)
{
    const long long r = at->r + 1;
    const int inside = r > 0 && at->row < trows; /* r == 0: from the prefix into cell 0 of row 0, which is where col and c already are */
    const int c = at->c + inside;
    const int next_cell = inside & (c == kind.cell) & (at->col + 1 < width), next_row = inside & (c >= kind.cell + kind.end);
    at->col = next_row ? 0 : at->col + next_cell;
    at->c = next_cell | next_row ? 0 : c;
    at->row += next_row;
    at->r = next_row ? 0 : r;
    return next_cell | next_row;
}

/* ---- who stores what ---- */

typedef struct
{
    unsigned head, tail;      /* bytes in front of the first 4-aligned address of the text, bytes behind the last word */
    unsigned long long words; /* aligned 32-bit words between them */
} trt_text_split;

TRT_TEXT_HD trt_text_split trt_text_split_of(unsigned long long address, unsigned long long bytes)
{
    trt_text_split s;
    s.head = (unsigned)((4 - (address & 3)) & 3);
    if (s.head > bytes)
        s.head = (unsigned)bytes;
    s.words = (bytes - s.head) / 4;
    s.tail = (unsigned)((bytes - s.head) % 4);
    return s;
}

/* waves of a text of `words` words: wave 0 is there for the lone bytes however short the text */
TRT_TEXT_HD unsigned long long trt_text_waves(const trt_text_kind kind, unsigned long long words)
{
    const unsigned long long waves = (words + (unsigned)kind.wave_words - 1) / (unsigned)kind.wave_words;
    return waves ? waves : 1;
}

/* the word lane `lane` of wave `wave` stores in its turn j < wave_words / 64; the wave's words are those below `words` */
TRT_TEXT_HD unsigned long long trt_text_lane_word(const trt_text_kind kind, unsigned long long wave, int lane, int j)
{
    return wave * (unsigned)kind.wave_words + (unsigned)(64 * j + lane);
}

/* the position of the byte that lane `lane` of wave 0 stores by itself, or -1: the head's bytes, lanes 0..2, and the tail's, lanes 4..6 */
TRT_TEXT_HD long long trt_text_lone_byte(const trt_text_split *s, int lane)
{
    if (lane < (int)s->head)
        return lane;
    if (lane >= 4 && lane - 4 < (int)s->tail)
        return (long long)(s->head + 4 * s->words) + (lane - 4);
    return -1;
}

#endif /* TRT_TEXT_MAP_H */
