/* trt_emit.c -- terminal emitter: framebuffer -> 24-bit ANSI background-colour cells, two spaces
 * per pixel (TRT.c:1084-1172).  The emitter stays on the host; it only fixes the integer
 * quantisation (int)(c*255) that the GPU frame must reproduce bit-exactly. */
#include <stdlib.h>
#include <string.h>

#include "trt_host.h"

static const char k_home[] = "\033[0;0H";                      /* reset_str, TRT.c:1102 */
static const char k_cell[] = "\033[48;2;000;000;000m  \033[0m"; /* pixel_str, TRT.c:1103 */
enum
{
    HOME_LEN = sizeof(k_home) - 1,  /* 6 */
    CELL_LEN = sizeof(k_cell) - 1,  /* 25 */
    RED_AT = 7,                     /* "\033[48;2;" */
    GREEN_AT = 11,
    BLUE_AT = 15
};

struct trt_emitter
{
    int width, height;
    size_t size;
    char *text;
};

int trt_emitter_create(int width, int height, trt_emitter **out)
{
    if (!out || width <= 0 || height <= 0)
        return TRT_HOST_ERR_ARGUMENT;
    *out = NULL;
    trt_emitter *e = (trt_emitter *)malloc(sizeof *e);
    if (!e)
        return TRT_HOST_ERR_MEMORY;
    e->width = width;
    e->height = height;
    /* sizeof(screenbuffer), TRT.c:1104: (sizeof(reset_str)+1) + ((sizeof(pixel_str)-1)*W + 1)*H + 1 */
    e->size = (sizeof(k_home) + 1) + ((size_t)CELL_LEN * width + 1) * height + 1;
    e->text = (char *)calloc(e->size, 1); /* static storage in the reference: the tail stays NUL */
    if (!e->text)
    {
        free(e);
        return TRT_HOST_ERR_MEMORY;
    }
    char *p = e->text;
    memcpy(p, k_home, HOME_LEN);
    p += HOME_LEN;
    for (int row = 0; row < height; row++)
    {
        for (int col = 0; col < width; col++, p += CELL_LEN)
            memcpy(p, k_cell, CELL_LEN);
        *p++ = '\n';
    }
    *out = e;
    return TRT_HOST_OK;
}

void trt_emitter_destroy(trt_emitter *e)
{
    if (e)
    {
        free(e->text);
        free(e);
    }
}

const char *trt_emitter_buffer(const trt_emitter *e) { return e ? e->text : NULL; }
size_t trt_emitter_size(const trt_emitter *e) { return e ? e->size : 0; }

/* byte_to_digits, TRT.c:1134-1139 (plain int arithmetic, also for out-of-range values) */
static void three_digits(char *at, int value)
{
    at[0] = (char)(value / 100 + '0');
    at[1] = (char)((value / 10) % 10 + '0');
    at[2] = (char)(value % 10 + '0');
}

int trt_emitter_patch(trt_emitter *e, const Screen *screen)
{
    /* the reference's buffer and Screen share SCREEN_WIDTH/HEIGHT (TRT.c:47-48, :1104); here they are run-time values
     * and must agree, or the walk below would leave the buffer */
    if (!e || !screen || !screen->pixels || screen->width != e->width || screen->height != e->height)
        return TRT_HOST_ERR_ARGUMENT;
    char *row_text = e->text + HOME_LEN;
    for (int row = 0; row < screen->height; row++, row_text += (size_t)CELL_LEN * e->width + 1)
    {
        char *cell = row_text;
        for (int col = 0; col < screen->width; col++, cell += CELL_LEN)
        {
            const Vector px = screen->pixels[row * screen->width + col];
            three_digits(cell + RED_AT, (int)(px.x * 255));
            three_digits(cell + GREEN_AT, (int)(px.y * 255));
            three_digits(cell + BLUE_AT, (int)(px.z * 255));
        }
    }
    return TRT_HOST_OK;
}

int trt_emitter_patch_rgb8(trt_emitter *e, const unsigned char *rgb)
{
    if (!e || !rgb)
        return TRT_HOST_ERR_ARGUMENT;
    char *row_text = e->text + HOME_LEN;
    for (int row = 0; row < e->height; row++, row_text += (size_t)CELL_LEN * e->width + 1)
    {
        char *cell = row_text;
        for (int col = 0; col < e->width; col++, cell += CELL_LEN, rgb += 3)
        {
            three_digits(cell + RED_AT, rgb[0]);
            three_digits(cell + GREEN_AT, rgb[1]);
            three_digits(cell + BLUE_AT, rgb[2]);
        }
    }
    return TRT_HOST_OK;
}

/* The delta text (csrc/trt_ansi_delta.h holds the format): the obvious walk, a cell at a time, on purpose without that header -- this
 * is what the header's arithmetic and the device kernels are held against. */
static const char k_goto[] = "\033[00000;00000H";
static const char k_reset[] = "\033[0m";
enum
{
    GOTO_LEN = sizeof(k_goto) - 1,   /* 14 */
    GOTO_ROW_AT = 2,
    GOTO_COLUMN_AT = 8,
    COLOUR_LEN = 19,                 /* pixel_str up to and including its 'm' */
    RESET_LEN = sizeof(k_reset) - 1, /* 4 */
    DELTA_MAX_ROWS = 99999,
    DELTA_MAX_WIDTH = 49999
};

static void five_digits(char *at, int value)
{
    for (int place = 4; place >= 0; place--, value /= 10)
        at[place] = (char)(value % 10 + '0');
}

int trt_emitter_delta_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!shown || !next || !text || !bytes || width <= 0 || rows <= 0 || width > DELTA_MAX_WIDTH || rows > DELTA_MAX_ROWS)
        return TRT_HOST_ERR_ARGUMENT;
    if (capacity < (size_t)rows * ((size_t)21 * width + 18))
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    for (int row = 0; row < rows; row++)
    {
        const unsigned char *was = shown + (size_t)row * width * 3, *now = next + (size_t)row * width * 3;
        int in_run = 0;
        for (int col = 0; col < width; col++)
        {
            const unsigned char *px = now + 3 * col;
            if (memcmp(was + 3 * col, px, 3) == 0)
                continue;
            if (!in_run)
            { /* the cursor to the cell's first column: rows and columns count from 1, a cell is two columns wide */
                memcpy(p, k_goto, GOTO_LEN);
                five_digits(p + GOTO_ROW_AT, row + 1);
                five_digits(p + GOTO_COLUMN_AT, 2 * col + 1);
                p += GOTO_LEN;
            }
            if (!in_run || memcmp(px - 3, px, 3) != 0)
            { /* the background colour, unless the cell painted just before has it */
                memcpy(p, k_cell, COLOUR_LEN);
                three_digits(p + RED_AT, px[0]);
                three_digits(p + GREEN_AT, px[1]);
                three_digits(p + BLUE_AT, px[2]);
                p += COLOUR_LEN;
            }
            *p++ = ' ';
            *p++ = ' ';
            in_run = col + 1 < width && memcmp(was + 3 * (col + 1), px + 3, 3) != 0;
            if (!in_run)
            {
                memcpy(p, k_reset, RESET_LEN);
                p += RESET_LEN;
            }
        }
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The half-block text (csrc/trt_ansi_half.h holds the format): two owned rows per line of text, the upper one as the foreground and the
 * lower one as the background colour of an upper-half-block glyph.  Plain loops, on purpose without that header -- this is what the
 * header's arithmetic and the device kernels are held against. */
static const char k_half_cell[] = "\033[38;2;000;000;000;48;2;000;000;000m\xe2\x96\x80";
static const char k_half_end[] = "\033[0m\n";
enum
{
    HALF_CELL_LEN = sizeof(k_half_cell) - 1, /* 39 */
    HALF_END_LEN = sizeof(k_half_end) - 1,   /* 5 */
    HALF_UPPER_AT = 7,                       /* "\033[38;2;" */
    HALF_LOWER_AT = 24                       /* ... "RRR;GGG;BBB;48;2;" */
};

int trt_emitter_half_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!rgb || !text || !bytes || width <= 0 || rows <= 0)
        return TRT_HOST_ERR_ARGUMENT;
    const size_t text_rows = ((size_t)rows + 1) / 2;
    if (capacity < HOME_LEN + ((size_t)HALF_CELL_LEN * width + HALF_END_LEN) * text_rows)
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    memcpy(p, k_home, HOME_LEN);
    p += HOME_LEN;
    for (int upper_row = 0; upper_row < rows; upper_row += 2)
    {
        const unsigned char *upper = rgb + (size_t)upper_row * width * 3;
        const unsigned char *lower = upper_row + 1 < rows ? upper + (size_t)width * 3 : NULL; /* behind an odd frame's last row: black */
        for (int col = 0; col < width; col++, p += HALF_CELL_LEN)
        {
            memcpy(p, k_half_cell, HALF_CELL_LEN);
            for (int ch = 0; ch < 3; ch++)
            {
                three_digits(p + HALF_UPPER_AT + 4 * ch, upper[3 * col + ch]);
                three_digits(p + HALF_LOWER_AT + 4 * ch, lower ? lower[3 * col + ch] : 0);
            }
        }
        memcpy(p, k_half_end, HALF_END_LEN);
        p += HALF_END_LEN;
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The half-block delta text (csrc/trt_ansi_delta_half.h holds the format): the delta's walk over the half-block text's cells, one
 * column each, the upper pixel's colour as the foreground and the lower one's as the background.  Plain loops, on purpose without
 * that header -- this is what the header's arithmetic and the device kernels are held against. */
static const char k_upper[] = "\033[38;2;000;000;000";
static const char k_lower[] = "48;2;000;000;000";
static const char k_glyph[] = "\xe2\x96\x80";
enum
{
    UPPER_LEN = sizeof(k_upper) - 1, /* 18 */
    LOWER_LEN = sizeof(k_lower) - 1, /* 16 */
    GLYPH_LEN = sizeof(k_glyph) - 1, /* 3 */
    DELTA_HALF_MAX_TEXT_ROWS = 99999,
    DELTA_HALF_MAX_WIDTH = 99999
};

int trt_emitter_delta_half_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    static const unsigned char black[3] = {0, 0, 0};
    if (!shown || !next || !text || !bytes || width <= 0 || rows <= 0 || width > DELTA_HALF_MAX_WIDTH || rows > 2 * DELTA_HALF_MAX_TEXT_ROWS)
        return TRT_HOST_ERR_ARGUMENT;
    const size_t text_rows = ((size_t)rows + 1) / 2;
    if (capacity < text_rows * ((size_t)39 * width + 18))
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    for (size_t t = 0; t < text_rows; t++)
    {
        const int has_lower = 2 * t + 1 < (size_t)rows; /* behind an odd frame's last row: black in both frames, and not read */
        const unsigned char *was_up = shown + 2 * t * width * 3, *now_up = next + 2 * t * width * 3;
        const unsigned char *was_low = has_lower ? was_up + (size_t)width * 3 : NULL, *now_low = has_lower ? now_up + (size_t)width * 3 : NULL;
        int in_run = 0;
        for (int col = 0; col < width; col++)
        {
            const unsigned char *up = now_up + 3 * col, *low = has_lower ? now_low + 3 * col : black;
            if (memcmp(was_up + 3 * col, up, 3) == 0 && (!has_lower || memcmp(was_low + 3 * col, low, 3) == 0))
                continue;
            if (!in_run)
            { /* the cursor to the cell: text rows and columns count from 1, a cell is one column wide */
                memcpy(p, k_goto, GOTO_LEN);
                five_digits(p + GOTO_ROW_AT, (int)t + 1);
                five_digits(p + GOTO_COLUMN_AT, col + 1);
                p += GOTO_LEN;
            }
            /* the colours, unless the cell painted just before has them */
            const int set_upper = !in_run || memcmp(up - 3, up, 3) != 0, set_lower = !in_run || (has_lower && memcmp(low - 3, low, 3) != 0);
            if (set_upper)
            {
                memcpy(p, k_upper, UPPER_LEN);
                for (int ch = 0; ch < 3; ch++)
                    three_digits(p + HALF_UPPER_AT + 4 * ch, up[ch]);
                p += UPPER_LEN;
            }
            if (set_lower)
            {
                *p++ = set_upper ? ';' : '\033';
                if (!set_upper)
                    *p++ = '[';
                memcpy(p, k_lower, LOWER_LEN);
                for (int ch = 0; ch < 3; ch++)
                    three_digits(p + 5 + 4 * ch, low[ch]);
                p += LOWER_LEN;
            }
            if (set_upper || set_lower)
                *p++ = 'm';
            memcpy(p, k_glyph, GLYPH_LEN);
            p += GLYPH_LEN;
            in_run = col + 1 < width &&
                     (memcmp(was_up + 3 * (col + 1), up + 3, 3) != 0 || (has_lower && memcmp(was_low + 3 * (col + 1), now_low + 3 * (col + 1), 3) != 0));
            if (!in_run)
            {
                memcpy(p, k_reset, RESET_LEN);
                p += RESET_LEN;
            }
        }
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The kitty graphics-protocol image (csrc/trt_kitty.h holds the format): base64 of the RGB bytes in APC escape sequences of at most 4096
 * characters.  Plain loops and a table, on purpose without that header -- this is what the header's arithmetic and the device kernels are
 * held against.  No terminal has yet shown this picture: the key list below is written from memory of the protocol. */
static const char k_kitty_header[] = "\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=00000,v=00000,m=0;";
static const char k_kitty_chunk[] = "\033_Gm=00;";
static const char k_kitty_end[] = "\033\\";
static const char k_base64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
enum
{
    KITTY_HEADER_LEN = sizeof(k_kitty_header) - 1, /* 48 */
    KITTY_CHUNK_LEN = sizeof(k_kitty_chunk) - 1,   /* 8 */
    KITTY_END_LEN = sizeof(k_kitty_end) - 1,       /* 2 */
    KITTY_WIDTH_AT = 30,
    KITTY_ROWS_AT = 38,
    KITTY_MORE_AT = 46,
    KITTY_CHUNK_MORE_AT = 6,
    KITTY_CHUNK_PIXELS = 1024, /* 4096 characters, the protocol's limit per escape */
    KITTY_MAX = 99999
};

int trt_emitter_kitty_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!rgb || !text || !bytes || width <= 0 || rows <= 0 || width > KITTY_MAX || rows > KITTY_MAX)
        return TRT_HOST_ERR_ARGUMENT;
    const size_t pixels = (size_t)width * (size_t)rows, chunks = (pixels + KITTY_CHUNK_PIXELS - 1) / KITTY_CHUNK_PIXELS;
    if (capacity < 4 * pixels + 10 * chunks + 46)
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    memcpy(p, k_home, HOME_LEN);
    p += HOME_LEN;
    for (size_t chunk = 0; chunk < chunks; chunk++)
    {
        const size_t from = chunk * KITTY_CHUNK_PIXELS, to = from + KITTY_CHUNK_PIXELS < pixels ? from + KITTY_CHUNK_PIXELS : pixels;
        const char more = (char)('0' + (chunk + 1 < chunks));
        if (chunk == 0)
        {
            memcpy(p, k_kitty_header, KITTY_HEADER_LEN);
            five_digits(p + KITTY_WIDTH_AT, width);
            five_digits(p + KITTY_ROWS_AT, rows);
            p[KITTY_MORE_AT] = more;
            p += KITTY_HEADER_LEN;
        }
        else
        {
            memcpy(p, k_kitty_chunk, KITTY_CHUNK_LEN);
            p[KITTY_CHUNK_MORE_AT] = more;
            p += KITTY_CHUNK_LEN;
        }
        for (size_t px = from; px < to; px++, p += 4)
        {
            const unsigned n = (unsigned)rgb[3 * px] << 16 | (unsigned)rgb[3 * px + 1] << 8 | (unsigned)rgb[3 * px + 2];
            p[0] = k_base64[n >> 18];
            p[1] = k_base64[n >> 12 & 63];
            p[2] = k_base64[n >> 6 & 63];
            p[3] = k_base64[n & 63];
        }
        memcpy(p, k_kitty_end, KITTY_END_LEN);
        p += KITTY_END_LEN;
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

int trt_emitter_write(const trt_emitter *e, FILE *stream)
{
    if (!e || !stream)
        return TRT_HOST_ERR_ARGUMENT;
    return fwrite(e->text, 1, e->size, stream) == e->size ? TRT_HOST_OK : TRT_HOST_ERR_OPEN;
}

int trt_draw_screen(const Screen *screen, FILE *stream)
{
    if (!screen || !screen->pixels || !stream)
        return TRT_HOST_ERR_ARGUMENT;
    if (fputs(k_home, stream) < 0)
        return TRT_HOST_ERR_OPEN;
    for (int row = 0; row < screen->height; row++)
    {
        for (int col = 0; col < screen->width; col++)
        {
            const Vector px = screen->pixels[row * screen->width + col];
            fprintf(stream, "\033[48;2;%d;%d;%dm  \033[0m", (int)(px.x * 255), (int)(px.y * 255), (int)(px.z * 255));
        }
        fputc('\n', stream);
    }
    return TRT_HOST_OK;
}

/* ---- the xterm 256-colour palette (csrc/trt_xterm256.h holds the rule and its closed form) ---- */

/* the closed form the device computes, compiled here from the header the kernels compile; the header's inline function has the name
 * this library exports, so it is compiled under another */
#define trt_xterm256_index trt_xterm256_index_closed_form
#include "../trt_xterm256.h"
#undef trt_xterm256_index

unsigned trt_xterm256_index(unsigned r, unsigned g, unsigned b)
{
    return trt_xterm256_index_closed_form(r & 0xffu, g & 0xffu, b & 0xffu);
}

/* The rule itself: all 240 fixed entries in index order -- the cube's 16 + 36 i + 6 j + k, then the ramp's 232 + k -- the first of the
 * nearest.  Plain loops, on purpose without the header's arithmetic -- this is what the closed form and the device kernels are held
 * against. */
unsigned trt_xterm256_index_search(unsigned r, unsigned g, unsigned b)
{
    static const int levels[6] = {0, 95, 135, 175, 215, 255};
    const int pr = (int)(r & 0xffu), pg = (int)(g & 0xffu), pb = (int)(b & 0xffu);
    unsigned best = 16, index = 16;
    int best_distance = 3 * 255 * 255 + 1; /* above every distance */
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++)
            for (int k = 0; k < 6; k++, index++)
            {
                const int distance = (pr - levels[i]) * (pr - levels[i]) + (pg - levels[j]) * (pg - levels[j]) + (pb - levels[k]) * (pb - levels[k]);
                if (distance < best_distance) /* strictly nearer: ties stay with the lower index */
                    best = index, best_distance = distance;
            }
    for (int k = 0; k < 24; k++, index++)
    {
        const int grey = 8 + 10 * k;
        const int distance = (pr - grey) * (pr - grey) + (pg - grey) * (pg - grey) + (pb - grey) * (pb - grey);
        if (distance < best_distance)
            best = index, best_distance = distance;
    }
    return best;
}

/* The full text in the palette (csrc/trt_ansi256.h holds the format): two spaces a pixel on the background colour the search finds. */
static const char k_cell256[] = "\033[48;5;000m  ";
static const char k_end256[] = "\033[0m\n";
static const char k_half_cell256[] = "\033[38;5;000;48;5;000m\xe2\x96\x80";
enum
{
    CELL256_LEN = sizeof(k_cell256) - 1,           /* 13 */
    END256_LEN = sizeof(k_end256) - 1,             /* 5 */
    HALF_CELL256_LEN = sizeof(k_half_cell256) - 1, /* 23 */
    INDEX256_AT = 7,                               /* "\033[48;5;" */
    UPPER256_AT = 7,                               /* "\033[38;5;" */
    LOWER256_AT = 16,                              /* ... "UUU;48;5;" */
    BLACK256 = 16
};

int trt_emitter_ansi256_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!rgb || !text || !bytes || width <= 0 || rows <= 0)
        return TRT_HOST_ERR_ARGUMENT;
    if (capacity < HOME_LEN + ((size_t)CELL256_LEN * width + END256_LEN) * (size_t)rows)
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    memcpy(p, k_home, HOME_LEN);
    p += HOME_LEN;
    for (int row = 0; row < rows; row++)
    {
        const unsigned char *px = rgb + (size_t)row * width * 3;
        for (int col = 0; col < width; col++, p += CELL256_LEN)
        {
            memcpy(p, k_cell256, CELL256_LEN);
            three_digits(p + INDEX256_AT, (int)trt_xterm256_index_search(px[3 * col], px[3 * col + 1], px[3 * col + 2]));
        }
        memcpy(p, k_end256, END256_LEN);
        p += END256_LEN;
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The half-block text in the palette (csrc/trt_ansi256_half.h holds the format): two owned rows per line of text, the upper one's index
 * as the foreground and the lower one's as the background of an upper-half-block glyph; black, 016, behind an odd frame's last row. */
int trt_emitter_ansi256_half_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!rgb || !text || !bytes || width <= 0 || rows <= 0)
        return TRT_HOST_ERR_ARGUMENT;
    const size_t text_rows = ((size_t)rows + 1) / 2;
    if (capacity < HOME_LEN + ((size_t)HALF_CELL256_LEN * width + END256_LEN) * text_rows)
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    memcpy(p, k_home, HOME_LEN);
    p += HOME_LEN;
    for (int upper_row = 0; upper_row < rows; upper_row += 2)
    {
        const unsigned char *upper = rgb + (size_t)upper_row * width * 3;
        const unsigned char *lower = upper_row + 1 < rows ? upper + (size_t)width * 3 : NULL;
        for (int col = 0; col < width; col++, p += HALF_CELL256_LEN)
        {
            memcpy(p, k_half_cell256, HALF_CELL256_LEN);
            three_digits(p + UPPER256_AT, (int)trt_xterm256_index_search(upper[3 * col], upper[3 * col + 1], upper[3 * col + 2]));
            three_digits(p + LOWER256_AT, lower ? (int)trt_xterm256_index_search(lower[3 * col], lower[3 * col + 1], lower[3 * col + 2]) : BLACK256);
        }
        memcpy(p, k_end256, END256_LEN);
        p += END256_LEN;
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The delta text in the palette (csrc/trt_ansi256_delta.h holds the format): trt_emitter_delta_rgb8's walk over the INDICES the search
 * finds -- a cell is changed where its index is, and "as the cell to the left" compares indices.  Plain loops, on purpose without that
 * header and without the closed form -- this is what the header's arithmetic and the device kernels are held against. */
static unsigned index256_at(const unsigned char *px) { return trt_xterm256_index_search(px[0], px[1], px[2]); }

enum
{
    COLOUR256_LEN = 11 /* the palette cell up to and including its 'm' */
};

int trt_emitter_delta256_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!shown || !next || !text || !bytes || width <= 0 || rows <= 0 || width > DELTA_MAX_WIDTH || rows > DELTA_MAX_ROWS)
        return TRT_HOST_ERR_ARGUMENT;
    if (capacity < (size_t)rows * ((size_t)13 * width + 13 + (size_t)5 * (((size_t)width + 1) / 2)))
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    for (int row = 0; row < rows; row++)
    {
        const unsigned char *was = shown + (size_t)row * width * 3, *now = next + (size_t)row * width * 3;
        int in_run = 0;
        for (int col = 0; col < width; col++)
        {
            const unsigned index = index256_at(now + 3 * col);
            if (index256_at(was + 3 * col) == index)
                continue;
            if (!in_run)
            { /* the cursor to the cell's first column: rows and columns count from 1, a cell is two columns wide */
                memcpy(p, k_goto, GOTO_LEN);
                five_digits(p + GOTO_ROW_AT, row + 1);
                five_digits(p + GOTO_COLUMN_AT, 2 * col + 1);
                p += GOTO_LEN;
            }
            if (!in_run || index256_at(now + 3 * (col - 1)) != index)
            { /* the background colour, unless the cell painted just before has it */
                memcpy(p, k_cell256, COLOUR256_LEN);
                three_digits(p + INDEX256_AT, (int)index);
                p += COLOUR256_LEN;
            }
            *p++ = ' ';
            *p++ = ' ';
            in_run = col + 1 < width && index256_at(was + 3 * (col + 1)) != index256_at(now + 3 * (col + 1));
            if (!in_run)
            {
                memcpy(p, k_reset, RESET_LEN);
                p += RESET_LEN;
            }
        }
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The half-block delta text in the palette (csrc/trt_ansi256_delta_half.h holds the format): trt_emitter_delta_half_rgb8's walk over the
 * indices the search finds; behind an odd frame's last row the lower index is black, 016, in both frames, and nothing there is read. */
static const char k_upper256[] = "\033[38;5;000";
static const char k_lower256[] = "48;5;000";
enum
{
    UPPER256_LEN = sizeof(k_upper256) - 1, /* 10 */
    LOWER256_LEN = sizeof(k_lower256) - 1  /* 8 */
};

int trt_emitter_delta256_half_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    if (!shown || !next || !text || !bytes || width <= 0 || rows <= 0 || width > DELTA_HALF_MAX_WIDTH || rows > 2 * DELTA_HALF_MAX_TEXT_ROWS)
        return TRT_HOST_ERR_ARGUMENT;
    const size_t text_rows = ((size_t)rows + 1) / 2;
    if (capacity < text_rows * ((size_t)23 * width + 18))
        return TRT_HOST_ERR_ARGUMENT;
    char *p = text;
    for (size_t t = 0; t < text_rows; t++)
    {
        const int has_lower = 2 * t + 1 < (size_t)rows;
        const unsigned char *was_up = shown + 2 * t * width * 3, *now_up = next + 2 * t * width * 3;
        const unsigned char *was_low = has_lower ? was_up + (size_t)width * 3 : NULL, *now_low = has_lower ? now_up + (size_t)width * 3 : NULL;
        int in_run = 0;
        for (int col = 0; col < width; col++)
        {
            const unsigned up = index256_at(now_up + 3 * col), low = has_lower ? index256_at(now_low + 3 * col) : BLACK256;
            if (index256_at(was_up + 3 * col) == up && (!has_lower || index256_at(was_low + 3 * col) == low))
                continue;
            if (!in_run)
            { /* the cursor to the cell: text rows and columns count from 1, a cell is one column wide */
                memcpy(p, k_goto, GOTO_LEN);
                five_digits(p + GOTO_ROW_AT, (int)t + 1);
                five_digits(p + GOTO_COLUMN_AT, col + 1);
                p += GOTO_LEN;
            }
            /* the colours, unless the cell painted just before has them */
            const int set_upper = !in_run || index256_at(now_up + 3 * (col - 1)) != up;
            const int set_lower = !in_run || (has_lower && index256_at(now_low + 3 * (col - 1)) != low);
            if (set_upper)
            {
                memcpy(p, k_upper256, UPPER256_LEN);
                three_digits(p + UPPER256_AT, (int)up);
                p += UPPER256_LEN;
            }
            if (set_lower)
            {
                *p++ = set_upper ? ';' : '\033';
                if (!set_upper)
                    *p++ = '[';
                memcpy(p, k_lower256, LOWER256_LEN);
                three_digits(p + 5, (int)low);
                p += LOWER256_LEN;
            }
            if (set_upper || set_lower)
                *p++ = 'm';
            memcpy(p, k_glyph, GLYPH_LEN);
            p += GLYPH_LEN;
            in_run = col + 1 < width && (index256_at(was_up + 3 * (col + 1)) != index256_at(now_up + 3 * (col + 1)) ||
                                         (has_lower && index256_at(was_low + 3 * (col + 1)) != index256_at(now_low + 3 * (col + 1))));
            if (!in_run)
            {
                memcpy(p, k_reset, RESET_LEN);
                p += RESET_LEN;
            }
        }
    }
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}

/* The DEC sixel image (csrc/trt_sixel.h holds the format): the 240 fixed palette entries as colour registers, then the picture in bands of
 * six pixel rows, a band one colour row per index that occurs in it.  Plain loops over the search, on purpose without that header -- this is
 * what the header's arithmetic and the device kernels are held against.  No terminal has shown this picture: the format is written from
 * memory of DEC's description. */
static const char k_sixel_dcs[] = "\033P0;1;0q";
static const char k_sixel_raster[] = "\"1;1;00000;00000";
static const char k_sixel_define[] = "#000;2;000;000;000";
static const char k_sixel_end[] = "\033\\";
enum
{
    SIXEL_DCS_LEN = sizeof(k_sixel_dcs) - 1,       /* 8 */
    SIXEL_RASTER_LEN = sizeof(k_sixel_raster) - 1, /* 16 */
    SIXEL_DEFINE_LEN = sizeof(k_sixel_define) - 1, /* 18 */
    SIXEL_END_LEN = sizeof(k_sixel_end) - 1,       /* 2 */
    SIXEL_WIDTH_AT = 5,
    SIXEL_ROWS_AT = 11,
    SIXEL_FIRST = 16,
    SIXEL_COLOURS = 240,
    SIXEL_BAND = 6,
    SIXEL_FIXED = HOME_LEN + SIXEL_DCS_LEN + SIXEL_RASTER_LEN + SIXEL_COLOURS * SIXEL_DEFINE_LEN + SIXEL_END_LEN, /* 4352 */
    SIXEL_MAX = 99999
};

/* the indices of band `band`'s pixels, band_rows x width, and which of the 240 occur; returns how many do */
static int sixel_band(const unsigned char *rgb, int width, int band, int band_rows, unsigned char *index, unsigned char *occurs)
{
    int colours = 0;
    memset(occurs, 0, SIXEL_COLOURS);
    for (int j = 0; j < band_rows; j++)
    {
        const unsigned char *px = rgb + (size_t)(SIXEL_BAND * band + j) * width * 3;
        for (int col = 0; col < width; col++)
        {
            const unsigned n = trt_xterm256_index_search(px[3 * col], px[3 * col + 1], px[3 * col + 2]);
            index[(size_t)j * width + col] = (unsigned char)n;
            colours += !occurs[n - SIXEL_FIRST];
            occurs[n - SIXEL_FIRST] = 1;
        }
    }
    return colours;
}

int trt_emitter_sixel_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes)
{
    static const int levels[6] = {0, 95, 135, 175, 215, 255};
    if (!rgb || !text || !bytes || width <= 0 || rows <= 0 || width > SIXEL_MAX || rows > SIXEL_MAX)
        return TRT_HOST_ERR_ARGUMENT;
    const int bands = (rows + SIXEL_BAND - 1) / SIXEL_BAND, pad = 1 + ((4 - (width + 1) % 4) % 4);
    const size_t row_len = 4 + (size_t)width + (size_t)pad;
    unsigned char occurs[SIXEL_COLOURS];
    unsigned char *index = (unsigned char *)malloc((size_t)SIXEL_BAND * width);
    if (!index)
        return TRT_HOST_ERR_MEMORY;
    /* a refused call writes nothing: where the capacity is below what any frame of the size fits into, the length first */
    size_t most = 0, colour_rows = 0;
    for (int band = 0; band < bands; band++)
    {
        const size_t pixels = (size_t)width * (size_t)(rows - SIXEL_BAND * band < SIXEL_BAND ? rows - SIXEL_BAND * band : SIXEL_BAND);
        most += pixels < SIXEL_COLOURS ? pixels : SIXEL_COLOURS;
    }
    if (capacity < SIXEL_FIXED + row_len * most)
    {
        for (int band = 0; band < bands; band++)
        {
            const int band_rows = rows - SIXEL_BAND * band < SIXEL_BAND ? rows - SIXEL_BAND * band : SIXEL_BAND;
            colour_rows += (size_t)sixel_band(rgb, width, band, band_rows, index, occurs);
        }
        if (capacity < SIXEL_FIXED + row_len * colour_rows)
        {
            free(index);
            return TRT_HOST_ERR_ARGUMENT;
        }
    }
    char *p = text;
    memcpy(p, k_home, HOME_LEN);
    p += HOME_LEN;
    memcpy(p, k_sixel_dcs, SIXEL_DCS_LEN);
    p += SIXEL_DCS_LEN;
    memcpy(p, k_sixel_raster, SIXEL_RASTER_LEN);
    five_digits(p + SIXEL_WIDTH_AT, width);
    five_digits(p + SIXEL_ROWS_AT, rows);
    p += SIXEL_RASTER_LEN;
    for (int n = SIXEL_FIRST; n < SIXEL_FIRST + SIXEL_COLOURS; n++, p += SIXEL_DEFINE_LEN)
    {
        const int c = n - SIXEL_FIRST, grey = 8 + 10 * (n - 232);
        const int value[3] = {n < 232 ? levels[c / 36] : grey, n < 232 ? levels[c / 6 % 6] : grey, n < 232 ? levels[c % 6] : grey};
        memcpy(p, k_sixel_define, SIXEL_DEFINE_LEN);
        three_digits(p + 1, n);
        for (int ch = 0; ch < 3; ch++)
            three_digits(p + 7 + 4 * ch, (100 * value[ch] + 127) / 255);
    }
    for (int band = 0; band < bands; band++)
    {
        const int band_rows = rows - SIXEL_BAND * band < SIXEL_BAND ? rows - SIXEL_BAND * band : SIXEL_BAND;
        int left = sixel_band(rgb, width, band, band_rows, index, occurs);
        for (int n = SIXEL_FIRST; n < SIXEL_FIRST + SIXEL_COLOURS; n++)
        {
            if (!occurs[n - SIXEL_FIRST])
                continue;
            left--;
            *p++ = '#';
            three_digits(p, n);
            p += 3;
            for (int col = 0; col < width; col++)
            {
                int six = 0;
                for (int j = 0; j < band_rows; j++)
                    six |= (index[(size_t)j * width + col] == n) << j;
                *p++ = (char)(63 + six);
            }
            for (int k = 0; k < pad - 1; k++)
                *p++ = '$';
            *p++ = left == 0 && band + 1 < bands ? '-' : '$';
        }
    }
    memcpy(p, k_sixel_end, SIXEL_END_LEN);
    p += SIXEL_END_LEN;
    free(index);
    *bytes = (size_t)(p - text);
    return TRT_HOST_OK;
}
