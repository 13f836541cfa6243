/*
 * trt_host.h -- host-side C companions of the frame producer: the pieces of the reference that sit
 * either side of project_scene() and stay on the CPU.
 *
 *   camera   per-frame orbit that produces the Camera input        TRT.c:290-305, 558-624, 1327-1336
 *   skybox   P6 reader + cubemap loader that produce the Skybox    TRT.c:309-436
 *   emitter  framebuffer -> 24-bit ANSI background-colour cells    TRT.c:1084-1172
 *
 * Plain C, no GPU calls; compiled into libtrt_hip.so next to the C-ABI of trt_hip.h.
 * Unlike the reference, nothing here calls exit(): errors come back as TRT_HOST_* codes.
 */
#ifndef TRT_HOST_H
#define TRT_HOST_H

#include <stdio.h>

#include "trt.h"

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    TRT_HOST_OK = 0,
    TRT_HOST_ERR_OPEN = -101,    /* TRT.c:318-322  "Error opening file" */
    TRT_HOST_ERR_FORMAT = -102,  /* TRT.c:327-332  not a P6 file / malformed header */
    TRT_HOST_ERR_MAXVAL = -103,  /* TRT.c:351-356  max colour value is not 255 */
    TRT_HOST_ERR_MEMORY = -104,  /* TRT.c:363-368 */
    TRT_HOST_ERR_SHAPE = -105,   /* TRT.c:413-417  faces must be square and equal */
    TRT_HOST_ERR_ARGUMENT = -106,
    TRT_HOST_ERR_TRUNCATED = -107 /* fewer than width*height*3 data bytes (the reference stores EOF bytes silently) */
};

/* ---- camera ------------------------------------------------------------------------------- */
void trt_init_frame(Frame *frame);                                    /* TRT.c:290 */
/* TRT.c:299: distance 1, height 5, width 5*aspect_w/aspect_h (the reference bakes 480/280) */
void trt_init_camera(Camera *camera, int aspect_w, int aspect_h);
void trt_rotate_basis(Basis *basis, const Basis *rotation);          /* TRT.c:558 */
void trt_rotate_basis_x(Basis *basis, double angle);                  /* TRT.c:576 */
void trt_rotate_basis_y(Basis *basis, double angle);                  /* TRT.c:586 */
void trt_rotate_basis_z(Basis *basis, double angle);                  /* TRT.c:596 */
void trt_transform_frame(Frame *frame, const Frame *transform);      /* TRT.c:607 */
/* TRT.c:1327-1336: frame of the orbiting camera at wall-clock second t (screen_* members untouched) */
void trt_orbit_camera(Camera *camera, double t);

/* ---- skybox ------------------------------------------------------------------------------- */
/* TRT.c:309.  *colors is malloc'ed (caller frees). */
int trt_read_ppm(const char *filename, Color **colors, int *width, int *height);
/* TRT.c:388.  directory holds +X.ppm -X.ppm +Y.ppm -Y.ppm +Z.ppm -Z.ppm (the reference's
 * "skybox/<name>").  On error nothing is left allocated and skybox->dim is -1. */
int trt_load_skybox(Skybox *skybox, const char *directory);
void trt_free_skybox(Skybox *skybox);                                 /* TRT.c:430 */

/* ---- emitter ------------------------------------------------------------------------------ */
typedef struct trt_emitter trt_emitter;
/* TRT.c:1102-1131: "\033[0;0H" then per row width cells "\033[48;2;RRR;GGG;BBBm  \033[0m" and '\n'.
 * The buffer has the reference's sizeof(screenbuffer) = 8 + (25*width+1)*height + 1 bytes. */
int trt_emitter_create(int width, int height, trt_emitter **out);
void trt_emitter_destroy(trt_emitter *e);
const char *trt_emitter_buffer(const trt_emitter *e);
size_t trt_emitter_size(const trt_emitter *e);
/* TRT.c:1142-1168: patch the 9 digits of every cell with (int)(c*255) (no output yet).  The Screen must have the
 * emitter's width and height (in the reference both come from SCREEN_WIDTH/HEIGHT): TRT_HOST_ERR_ARGUMENT otherwise. */
int trt_emitter_patch(trt_emitter *e, const Screen *screen);
/* the same from bytes already quantised on the GPU (trt_quantize_device): 3 bytes per pixel, width*height pixels */
int trt_emitter_patch_rgb8(trt_emitter *e, const unsigned char *rgb);
/* The DELTA text between two frames of such bytes (rows x width x 3 each): what a terminal that shows `shown` must be written to show
 * `next`.  The reference has no such emitter; the format is the project's own (csrc/trt_ansi_delta.h).  Per changed cell,
 * rows ascending, left to right: "\033[RRRRR;CCCCCH" (row + 1, 2 * column + 1) where a run of changed cells of one row starts,
 * "\033[48;2;RRR;GGG;BBBm" where a run starts or the colour differs from the cell's to the left, two spaces, and "\033[0m" where the run
 * ends.  No prefix, no newline, no NUL: equal frames give *bytes = 0.  At most rows * (21 * width + 18) bytes, which `capacity` must
 * hold; rows <= 99999, width <= 49999.  The sequential statement the device kernels (trt_render_device_ansi_delta, trt_hip.h) are
 * tested against, and the emitter of hosts that fetch RGB8 bytes.  TRT_HOST_ERR_ARGUMENT: NULL, a size that is not positive or above
 * the limits, a capacity below the bound. */
int trt_emitter_delta_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity,
                           size_t *bytes);
/* The HALF-BLOCK text of a frame of such bytes (rows x width x 3): two owned rows per line of text, one column and half a line per
 * pixel.  The reference has no such emitter; the format is the project's own (csrc/trt_ansi_half.h).  "\033[0;0H"; per text
 * row i < (rows + 1) / 2, width cells "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm" and the glyph U+2580 in UTF-8 (E2 96 80) -- RRR;GGG;BBB
 * the bytes of row 2 i (the foreground: the upper half), rrr;ggg;bbb those of row 2 i + 1 (the background: the lower half; 000;000;000
 * behind the last row of an odd frame) -- then "\033[0m\n".  No NUL: *bytes = 6 + (39 * width + 5) * ((rows + 1) / 2), which `capacity`
 * must hold.  The sequential statement the device kernels (trt_render_device_ansi_half, trt_hip.h) are tested against, and the emitter
 * of hosts that fetch RGB8 bytes.  TRT_HOST_ERR_ARGUMENT: NULL, a size that is not positive, a capacity below the length. */
int trt_emitter_half_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes);
/* The DELTA text between two such frames in HALF-BLOCK cells: what a terminal that shows `shown` as the half-block text must be written
 * to show `next`.  The format is the project's own (csrc/trt_ansi_delta_half.h).  A cell of text row t < (rows + 1) / 2
 * has the pixels of rows 2 t and 2 t + 1 (black behind an odd frame's last row, in both frames, and not read) and is changed when either
 * differs.  Per changed cell, text rows ascending, left to right: "\033[RRRRR;CCCCCH" (text row + 1, column + 1: a cell is one column
 * wide) where a run of changed cells of one text row starts; the colours that differ from the cell's to the left (both where a run
 * starts): "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm", "\033[38;2;RRR;GGG;BBBm", "\033[48;2;rrr;ggg;bbbm" or nothing; the glyph E2 96 80;
 * and "\033[0m" where the run ends.  No prefix, no newline, no NUL: equal frames give *bytes = 0.  At most
 * ((rows + 1) / 2) * (39 * width + 18) bytes, which `capacity` must hold; width <= 99999, rows <= 199998.  The sequential statement the
 * device kernels (trt_render_device_ansi_delta_half, trt_hip.h) are tested against.  TRT_HOST_ERR_ARGUMENT: NULL, a size that is not
 * positive or above the limits, a capacity below the bound. */
int trt_emitter_delta_half_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity,
                                size_t *bytes);
/* The frame of such bytes (rows x width x 3) as a KITTY GRAPHICS-PROTOCOL image, for terminals that take true pixels: base64 of the RGB
 * bytes, four characters a pixel, in APC escape sequences of at most 4096 characters.  The format is the project's own statement of the
 * protocol (csrc/trt_kitty.h) and NO TERMINAL HAS YET SHOWN IT.  "\033[0;0H"; then, P = width * rows pixels in row order cut
 * into K = ceil(P / 1024) chunks, "\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=WWWWW,v=RRRRR,m=M;" (five zero-padded digits each) in front of the first
 * chunk's characters and "\033_Gm=0M;" in front of every later chunk's, "\033\\" behind each; M is 1 but in the last chunk, where it is 0.
 * No '=', no newline, no NUL: *bytes = 4 P + 10 K + 46, which `capacity` must hold; width <= 99999, rows <= 99999.  The sequential
 * statement the device kernels (trt_render_device_kitty, trt_hip.h) are tested against, and the emitter of hosts that fetch RGB8 bytes.
 * TRT_HOST_ERR_ARGUMENT: NULL, a size that is not positive or above the limits, a capacity below the length. */
int trt_emitter_kitty_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes);
/* The xterm 256-colour palette, for terminals without 24-bit colour.  Entries 0..15 are the user's to theme and are never produced; of
 * the 240 fixed ones -- 16 + 36 i + 6 j + k the colour (L[i], L[j], L[k]), L = {0, 95, 135, 175, 215, 255}, and 232 + k the grey 8 + 10 k
 * -- a colour of three bytes has the entry with the least squared Euclidean distance in RGB bytes, ties to the lowest index.  No
 * dithering: the index depends on the three bytes alone.  trt_xterm256_index_search IS that rule, a loop over the 240 entries;
 * trt_xterm256_index is the closed form of csrc/trt_xterm256.h that the device kernels compute, compiled for the host: the two are equal
 * on all 2^24 colours.  Both take bytes (the low 8 bits of each argument) and return 16..255.  (A program that compiles
 * csrc/trt_xterm256.h itself, in front of this header, has trt_xterm256_index as that header's inline function.) */
#ifndef TRT_XTERM256_H
unsigned trt_xterm256_index(unsigned r, unsigned g, unsigned b);
#endif
unsigned trt_xterm256_index_search(unsigned r, unsigned g, unsigned b);
/* The frame of such bytes (rows x width x 3) as text in that palette: "\033[0;0H"; per row, width cells "\033[48;5;NNNm" and two spaces,
 * NNN the pixel's index by the SEARCH, three zero-padded digits; then "\033[0m\n".  No NUL: *bytes = 6 + (13 * width + 5) * rows, which
 * `capacity` must hold.  The format is the project's own (csrc/trt_ansi256.h).  The sequential statement the device kernels
 * (trt_render_device_ansi256, trt_hip.h) are tested against, and the emitter of hosts that fetch RGB8 bytes.  TRT_HOST_ERR_ARGUMENT: NULL,
 * a size that is not positive, a capacity below the length. */
int trt_emitter_ansi256_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes);
/* The same frame as HALF-BLOCK text in that palette (csrc/trt_ansi256_half.h): per text row t < (rows + 1) / 2, width cells
 * "\033[38;5;UUU;48;5;LLLm" and the glyph U+2580 in UTF-8 (E2 96 80) -- UUU the index of row 2 t, LLL that of row 2 t + 1; 016, black, behind
 * the last row of an odd frame -- then "\033[0m\n".  No NUL: *bytes = 6 + (23 * width + 5) * ((rows + 1) / 2).  Errors as above. */
int trt_emitter_ansi256_half_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes);
/* The DELTA text in that palette (csrc/trt_ansi256_delta.h): what a terminal that shows `shown` as trt_emitter_ansi256_rgb8's text must be
 * sent to show `next`.  A pixel's index is the SEARCH's; a cell is CHANGED when its index differs between the frames, not when a byte
 * does.  Per changed cell, rows ascending, left to right: "\033[RRRRR;CCCCCH" (row + 1, 2 * column + 1) where a run of changed cells of one
 * row starts, "\033[48;5;NNNm" where a run starts or the index differs from the new index of the cell to the left, two spaces, and "\033[0m"
 * where the run ends.  No NUL; frames of equal indices give *bytes = 0.  At most rows * (13 * width + 13 + 5 * ((width + 1) / 2)) bytes
 * -- every other cell changed: here more runs cost more --, which `capacity` must hold; rows <= 99999, width <= 49999.  The sequential
 * statement the device kernels (trt_render_device_ansi256_delta, trt_hip.h) are tested against.  TRT_HOST_ERR_ARGUMENT: NULL, a size
 * that is not positive or above the limits, a capacity below the bound. */
int trt_emitter_delta256_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity,
                              size_t *bytes);
/* The same in HALF-BLOCK cells (csrc/trt_ansi256_delta_half.h), for a terminal that shows trt_emitter_ansi256_half_rgb8's text: a cell of
 * text row t < (rows + 1) / 2 has the indices of rows 2 t and 2 t + 1 (016 behind an odd frame's last row, in both frames, and not read)
 * and is changed when either differs.  Per changed cell: "\033[RRRRR;CCCCCH" (text row + 1, column + 1) where a run starts; the colours
 * that differ from the left neighbour's new ones -- "\033[38;5;UUU;48;5;LLLm" where a run starts or both do, "\033[38;5;UUUm" or
 * "\033[48;5;LLLm" where one does, nothing where neither does --; the glyph E2 96 80; "\033[0m" where the run ends.  At most
 * ((rows + 1) / 2) * (23 * width + 18) bytes, which `capacity` must hold; width <= 99999, (rows + 1) / 2 <= 99999.  Errors as above. */
int trt_emitter_delta256_half_rgb8(const unsigned char *shown, const unsigned char *next, int width, int rows, char *text, size_t capacity,
                                   size_t *bytes);
/* The frame of such bytes (rows x width x 3) as a DEC SIXEL image, for the terminals that take sixel and not the kitty protocol (xterm,
 * foot, mlterm, Windows Terminal, VS Code's terminal, contour, tmux built with sixel).  The format is the project's own statement
 * (csrc/trt_sixel.h), written from memory of DEC's description, and NO TERMINAL HAS SHOWN IT.  "\033[0;0H"; "\033P0;1;0q";
 * "\"1;1;WWWWW;RRRRR" (five zero-padded digits each); the 240 colour registers "#NNN;2;PPP;PPP;PPP", NNN = 016..255 the xterm palette's
 * entry in RGB per cent, PPP = (100 v + 127) / 255; then per band of six rows, per index that a pixel of the band has BY THE SEARCH,
 * ascending, a colour row "#NNN", width characters 63 + (bit j: the pixel of the band's row j in this column has the index), T - 1 times "$"
 * and one more byte, "-" behind the last colour of every band but the last and "$" elsewhere, T = 1 + ((-(width + 1)) mod 4); then "\033\\".
 * No NUL, no newline: *bytes = 4352 + (4 + width + T) * (the colour rows), which depends on the picture and which `capacity` must hold;
 * width <= 99999, rows <= 99999.  The sequential statement the device kernels (trt_render_device_sixel, trt_hip.h) are tested against, and
 * the emitter of hosts that fetch RGB8 bytes.  TRT_HOST_ERR_ARGUMENT: NULL, a size that is not positive or above the limits, a capacity
 * below the length; a refused call writes nothing.  TRT_HOST_ERR_MEMORY: no room for the six rows of indices it works on. */
int trt_emitter_sixel_rgb8(const unsigned char *rgb, int width, int rows, char *text, size_t capacity, size_t *bytes);
/* TRT.c:1171: one fwrite of the whole buffer (trailing NULs included, as the reference does) */
int trt_emitter_write(const trt_emitter *e, FILE *stream);
/* TRT.c:1084-1099: the unbuffered printf form */
int trt_draw_screen(const Screen *screen, FILE *stream);

/* ---- frame fingerprint ------------------------------------------------------------------ */
/* FNV-1a-64 with the offset SURVEY.md 8c states, 1469598103934665603 (NOT the textbook 14695981039346656037), and prime
 * 1099511628211, over raw bytes: the hash the golden frames are recorded with, e.g. over screen->pixels[0 .. W*H) after project_scene (TRT.c:966). */
unsigned long long trt_fnv1a64(const void *data, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
