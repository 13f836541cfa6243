/*
 * trt_hip.h -- C-ABI of libtrt_hip.so, the MI355X (gfx950) frame producer.
 *
 * Plain C: pointers, ints and the structs of trt.h.  No C++/torch types cross it.
 * Each entry cites the reference interface it replaces or serves
 * ("TRT.c:N" = TerminalRayTracer.c line N of david-andrew/TerminalRayTracer).
 *
 * Two layers:
 *   1. drop-in          project_scene()            -- same symbol, same signature as TRT.c:966
 *   2. extended/context trt_*                      -- run-time bounce limit / rays per pixel
 *      (macros in the reference, TRT.c:54,58), device-resident framebuffers for off-screen
 *      rendering, row-tile sharding for multi-GPU, RGB8 quantisation for the emitter.
 *
 * This header is the PRODUCT boundary: the drop-in entries, the context API a host renders through, the tuning setters, the
 * multi-GPU entries.  What exists for the tests and the measurements only -- counters, table read-backs, self-tests, single-ray
 * probes, the RCCL stand-in hook -- is declared in include/trt_hip_diag.h; a host must not depend on it.
 *
 * All functions returning int return TRT_OK (0) or a negative TRT_ERR_*; trt_last_error()
 * gives the message.  A context is bound to one device and one stream and is not
 * thread-safe; separate contexts are independent.  The drop-in layer (project_scene, trt_render_frame,
 * trt_init/shutdown, trt_upload/invalidate_skybox) shares one default context and takes a lock: like the
 * reference's pure function it may be called from several threads, the calls then take turns.
 */
#ifndef TRT_HIP_H
#define TRT_HIP_H

#include "trt.h"

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    TRT_OK = 0,
    TRT_ERR_HIP = -1,         /* a HIP runtime call failed */
    TRT_ERR_ARGUMENT = -2,    /* NULL / out-of-range argument */
    TRT_ERR_NO_SCENE = -3,    /* render before trt_set_scene */
    TRT_ERR_CAPACITY = -4,    /* output buffer too small; a scene too large for LDS with trt_set_scene_image(ctx, 0) or the refraction extension */
    TRT_ERR_NOT_INITIALISED = -5
};

/* ---- 1. drop-in ------------------------------------------------------------------------------ */

/* Replaces `void project_scene(Scene *scene, Screen *screen)` (TRT.c:966; caller TRT.c:1339).
 * Same semantics at the reference's compile-time constants BOUNCE_LIMIT=10, RAYS_PER_PIXEL=10:
 * reads *scene (host pointers inside), overwrites screen->pixels[0 .. width*height).
 * Lazily creates a default context on device 0.  Any number of spheres and lights, as the reference: a scene whose image
 * does not fit LDS is read from device memory.  void like the original: a HIP failure prints
 * the error and aborts (the reference cannot fail here either). */
void project_scene(Scene *scene, Screen *screen);

/* project_scene with the two macros as run-time values (TRT.c:54, TRT.c:58).  Host in, host out. */
int trt_render_frame(const Scene *scene, Screen *screen, int bounce_limit, int rays_per_pixel);
/* The same entry under the name BASELINE.json's north_star gives it ("render_frame() entry"; the reference itself has no such
 * symbol: its frame producer is project_scene, TRT.c:966). */
int render_frame(const Scene *scene, Screen *screen, int bounce_limit, int rays_per_pixel);

/* The same frame as the bytes the emitter makes of it: rgb[(row*width + col)*3 + channel] = (int)(colour*255), the
 * conversion of buffered_draw_screen (TRT.c:1157-1163) done on the device, so that 3 bytes per pixel cross PCIe instead of 24.
 * For hosts whose only consumer of the frame is the terminal emitter (trt_emitter_patch_rgb8, trt_host.h).  Colours outside
 * [0, 1) convert as the reference's cast does on x86-64. */
int trt_render_frame_rgb8(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, unsigned char *rgb);

/* The same frame as the TEXT the emitter makes of it: what buffered_draw_screen (TRT.c:1142-1172) writes to the terminal -- "\033[0;0H", per
 * row `width` cells "\033[48;2;RRR;GGG;BBBm  \033[0m" and a newline, three NUL bytes -- formatted on the device by the pass that forms the
 * ordered mean.  text holds trt_ansi_bytes(width, height) bytes, the whole of which the host writes with one fwrite: byte for byte the
 * buffer of a trt_emitter (trt_host.h) after trt_emitter_patch_rgb8 of trt_render_frame_rgb8's bytes.  Lock and scene policy as above. */
int trt_render_frame_ansi(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text);

/* The same frame as the HALF-BLOCK text (trt_render_host_ansi_half below, on the default context: its format): two pixel rows per line of
 * text, one terminal column by half a line per pixel, for a terminal in a UTF-8 locale.  text holds trt_ansi_half_bytes(width, height)
 * bytes, the whole of which the host writes with one fwrite: byte for byte trt_emitter_half_rgb8 (trt_host.h) of trt_render_frame_rgb8's
 * bytes.  Lock and scene policy as above. */
int trt_render_frame_ansi_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text);

/* The same frame as a KITTY GRAPHICS-PROTOCOL image (trt_render_host_kitty below, on the default context: its format and its caveat -- no
 * terminal has yet shown it): true pixels, four bytes of text each, for a terminal that takes them.  text holds trt_kitty_bytes(width,
 * height) bytes, the whole of which the host writes with one fwrite: byte for byte trt_emitter_kitty_rgb8 (trt_host.h) of
 * trt_render_frame_rgb8's bytes.  width and height are at most 99999.  Lock and scene policy as above. */
int trt_render_frame_kitty(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text);

/* The same frame as the text in the XTERM 256-COLOUR PALETTE, for terminals without 24-bit colour (trt_render_host_ansi256 below, on the
 * default context: its format and its palette rule): two spaces a pixel, 13 bytes each.  text holds trt_ansi256_bytes(width, height)
 * bytes, the whole of which the host writes with one fwrite: byte for byte trt_emitter_ansi256_rgb8 (trt_host.h) of
 * trt_render_frame_rgb8's bytes.  Lock and scene policy as above. */
int trt_render_frame_ansi256(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text);

/* The same frame as the HALF-BLOCK text in the xterm 256-colour palette (trt_render_host_ansi256_half below, on the default context): two
 * pixel rows per line of text, 23 bytes a cell.  text holds trt_ansi256_half_bytes(width, height) bytes: byte for byte
 * trt_emitter_ansi256_half_rgb8 (trt_host.h) of trt_render_frame_rgb8's bytes.  The terminal must be in a UTF-8 locale.  Lock and scene
 * policy as above. */
int trt_render_frame_ansi256_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text);

/* The frame as the DELTA text against the frame this entry returned before (trt_render_host_ansi_delta below, on the default context: its
 * format, its rules for the host and its errors).  The first call, the first call of another size and the first call after trt_shutdown
 * return a keyframe: trt_render_frame_ansi's text.  text holds capacity_bytes >= trt_ansi_delta_capacity(width, height) bytes; the host
 * writes *bytes of them.  Lock and scene policy as above: the scene may change between calls, the delta is between the two frames. */
int trt_render_frame_ansi_delta(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text,
                                size_t capacity_bytes, size_t *bytes);

/* The same in HALF-BLOCK cells (trt_render_host_ansi_delta_half below, on the default context): the keyframe is
 * trt_render_frame_ansi_half's text, capacity_bytes >= trt_ansi_delta_half_capacity(width, height).  The default context keeps ONE shown
 * frame: a call of this entry after one of trt_render_frame_ansi_delta, or the other way round, returns a keyframe. */
int trt_render_frame_ansi_delta_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text,
                                     size_t capacity_bytes, size_t *bytes);

/* The two in the XTERM 256-COLOUR PALETTE (trt_render_host_ansi256_delta and trt_render_host_ansi256_delta_half below, on the default
 * context: their formats -- a cell is changed where its palette INDEX is -- and their rules): the keyframe is trt_render_frame_ansi256's
 * or trt_render_frame_ansi256_half's text, capacity_bytes >= trt_ansi256_delta_capacity / trt_ansi256_delta_half_capacity(width,
 * height).  The one shown frame remembers which of the FOUR kinds it was sent as: a call of any other kind returns a keyframe. */
extern int trt_render_frame_ansi256_delta(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text,
                                          size_t capacity_bytes, size_t *bytes);
extern int trt_render_frame_ansi256_delta_half(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text,
                                               size_t capacity_bytes, size_t *bytes);

/* The frame as a DEC SIXEL image (trt_render_host_sixel below, on the default context: its format and its caveat -- no terminal has shown
 * it): true pixels in the 240 fixed colours of the xterm palette, for the terminals that take sixel and not the kitty protocol.  The
 * length depends on the picture: text holds capacity_bytes >= trt_sixel_capacity(width, height) bytes, the host writes *bytes of them
 * with one fwrite: byte for byte trt_emitter_sixel_rgb8 (trt_host.h) of trt_render_frame_rgb8's bytes.  width and height are at most
 * 99999.  It neither reads nor changes the delta entries' shown frame.  Lock and scene policy as above. */
int trt_render_frame_sixel(const Scene *scene, int width, int height, int bounce_limit, int rays_per_pixel, char *text,
                           size_t capacity_bytes, size_t *bytes);

/* project_scene is a pure function of *scene (TRT.c:966): a caller may move a sphere before every call.  The drop-in entries
 * compare the primitives with the previous call's; a scene that has changed on `moving_after` consecutive calls counts as MOVING
 * and its candidate tables are rebuilt per call the cheap way (one family per sphere instead of 24 patches: ~4 ms instead of ~100 ms
 * at 256 spheres), and after `still_after` consecutive unchanged calls the full tables are built once.  moving_after = 0: every
 * change builds the full tables, and a scene that counts as moving when this is set stops doing so at once (its next call builds
 * the full tables).  What counts as a change: the spheres, either light array, or the ground's point or normal differ bytewise from
 * the previous call's; camera, ground materials, skybox, frame size, bounce limit and rays per pixel do not.  Defaults 2 and 3.
 * Frames are bit-identical whichever tables serve them.
 * trt_scene_is_moving: 1 while the default context treats its scene as moving. */
int trt_set_scene_policy(int moving_after, int still_after);
int trt_scene_is_moving(void);

/* Default-context management for the two calls above.  trt_init is optional (device 0 otherwise). */
int trt_init(int device);
int trt_shutdown(void);

/* Pre-upload a cubemap for the default context (what load_skybox, TRT.c:388, produced).  The
 * default context otherwise uploads on first use and re-uploads only when the face pointers, the
 * dimension, a stamp of sampled texels or trt_invalidate_skybox() say the texels changed.  The stamp
 * hashes about 256 texels of every face at a fixed stride (texel 0 of each face among them) and the
 * last texel of the last face, on every call: an image loaded into the same allocation shows.  Texels
 * edited in place that the stamp does not sample are NOT noticed: call trt_invalidate_skybox(). */
int trt_upload_skybox(const Skybox *skybox);
int trt_invalidate_skybox(void);

/* ---- 2. context API (device-resident) --------------------------------------------------------- */

typedef struct trt_context trt_context;

/* Rows of a W x H frame owned by one renderer, as interleaved row tiles: tiles of `tile_rows`
 * rows, this renderer owns tiles tile_first, tile_first+tile_step, ...  The renderer's
 * framebuffer is compact: owned rows in ascending order, `width` pixels each.
 * Whole frame: {W, H, H, 0, 1}. */
typedef struct
{
    int width;
    int height;
    int tile_rows;
    int tile_first;
    int tile_step;
} trt_rowset;

/* number of frame rows a rowset owns (0 on invalid input) */
int trt_rowset_rows(const trt_rowset *rows);
/* frame row of local row i, or -1 */
int trt_rowset_frame_row(const trt_rowset *rows, int local_row);

int trt_create(int device, trt_context **out);
int trt_destroy(trt_context *ctx);

/* Use an existing HIP stream (hipStream_t passed as void*; NULL = the context's own stream).
 * PyTorch callers pass torch.cuda.current_stream().cuda_stream. */
int trt_set_stream(trt_context *ctx, void *hip_stream);

/* Keep `reserved` compute units free of this context's kernels: its own stream is re-created with a CU mask and the
 * persistent kernel is sized for the remaining CUs.  The frame producer's workgroups are persistent and hold every
 * wave slot they are given until the frame ends; a collective that has to run beside them (the RCCL gather of the
 * previous frame in a multi-GPU run) would otherwise wait for a frame to drain.  Applies to the context's own stream
 * (not to one handed in with trt_set_stream); 0 removes the mask.  trt_get_stream returns the stream in use, e.g. to
 * wrap it for event synchronisation (torch.cuda.ExternalStream). */
int trt_reserve_cus(trt_context *ctx, int reserved);
int trt_get_stream(trt_context *ctx, void **hip_stream);

/* Upload everything of *scene except the camera: spheres, ground, lights, skybox texels.
 * (Scene layout TRT.c:196-208.)  Synchronous; call once per scene, not per frame. */
int trt_set_scene(trt_context *ctx, const Scene *scene);

/* `dst` renders the scene `src` was given, FROM src's tables: spheres, lights, cubemap and every candidate table of the scene stay
 * one copy per device however many contexts render it (the frame slots of a trt_dist render different cameras of one scene at the
 * same time: TRT.c:1296-1306 builds the scene once, TRT.c:1327-1339 moves the camera per frame).  Only what depends on the camera
 * -- the two tables of the eye's families -- and the per-frame buffers are dst's own.  Both contexts must be of the same device;
 * up to 8 contexts per scene, all of them driven from ONE thread (the slots a scene's sharers take and give back are not locked: a
 * trt_dist drives its frame slots from the thread that calls it).  While tables are shared, the table setters (trt_set_light_grids / _slabs, trt_set_path_grids /
 * _patches / _min_spheres) refuse on every sharer; trt_set_scene gives a context tables of its own again.  The refraction
 * extension's indices are per context (dst starts with none). */
int trt_share_scene(trt_context *dst, trt_context *src);
/* Device memory held by the scene's primitives and tables (bytes), how many contexts share them, host seconds of the last build. */
int trt_scene_info(trt_context *ctx, unsigned long long *table_bytes, int *sharers, double *build_seconds);

/* Render the owned rows into DEVICE memory: d_pixels[local_row*width + col] = 3 doubles
 * (the Screen layout of TRT.c:188-193).  Asynchronous on the context's stream.
 * camera: TRT.c:178-184, by value per frame as main() does (TRT.c:1327-1339). */
int trt_render_device(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                      int rays_per_pixel, void *d_pixels, size_t capacity_bytes);

/* trt_render_device as the emitter's bytes: d_rgb8[(local_row*width + col)*3 + channel] = (int)(c*255) (TRT.c:1157-1163), written
 * by the pass that forms the ordered mean over a pixel's samples -- no framebuffer of doubles is written or read on the way (the
 * reference-order kernel, trt_set_kernel(ctx, 1), has no such pass: its frame goes through a framebuffer of the context's and
 * trt_quantize_device's kernel).  Byte for byte what trt_render_device followed by trt_quantize_device gives.  d_rgb8 may have any
 * alignment; capacity_bytes counts bytes of RGB8 (owned rows * width * 3); errors as trt_render_device.  Asynchronous on the context's
 * stream.  One entry of trt_kernel_times; trt_render_kernel_times reports the pass as reduce_ms. */
int trt_render_device_rgb8(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                           int rays_per_pixel, void *d_rgb8, size_t capacity_bytes);

/* (int)(c*255) per channel (TRT.c:1157-1163) on the device: 3 bytes per pixel. Asynchronous. */
int trt_quantize_device(trt_context *ctx, const void *d_pixels, size_t num_pixels, void *d_rgb8);

/* Length of the terminal's text of a screen of `width` x `rows` owned rows: 8 + (25 * width + 1) * rows + 1 (sizeof(screenbuffer),
 * TRT.c:1104; trt_emitter_size for every size), 0 unless both are positive. */
size_t trt_ansi_bytes(int width, int rows);

/* trt_render_device as the terminal's text: the 6 bytes "\033[0;0H"; per owned row, in ascending order, `width` cells of 25 bytes
 * "\033[48;2;RRR;GGG;BBBm  \033[0m" and '\n'; three NUL bytes -- trt_ansi_bytes(width, owned rows) bytes, what trt_emitter_create(width,
 * owned rows) and trt_emitter_patch_rgb8 of trt_render_device_rgb8's bytes leave in trt_emitter_buffer; for the whole frame the reference's
 * screenbuffer.  Written by the pass that forms the ordered mean: neither doubles nor RGB8 bytes are written on the way, every byte of the
 * text is stored exactly once (d_text need not be initialised) and none outside it (the reference-order kernel, trt_set_kernel(ctx, 1),
 * goes through a framebuffer and bytes of the context's).  d_text may have any alignment; capacity_bytes counts bytes of text, to the
 * byte; checks and errors as trt_render_device_rgb8.  Asynchronous on the context's stream.  One entry of trt_kernel_times;
 * trt_render_kernel_times reports the pass as reduce_ms. */
int trt_render_device_ansi(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                           int rays_per_pixel, void *d_text, size_t capacity_bytes);

/* The formatting alone, of a frame that exists as RGB8 bytes in device memory (d_rgb8[(row*width + col)*3 + channel], e.g. what rank 0 of
 * a trt_dist_render_rgb8 gather holds): trt_ansi_bytes(width, rows) bytes at d_text, any alignment.  Asynchronous on the context's stream. */
int trt_ansi_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text);

/* ---- the half-block text: two pixel rows per line of text ---------------------------------------------------------------------
 * The text above paints a pixel as two spaces on a background colour: two terminal columns and a whole line, 25 bytes.  The HALF-BLOCK
 * text paints TWO pixels per character cell with the glyph U+2580 (upper half block; E2 96 80 in UTF-8, so the terminal must be in a
 * UTF-8 locale): the foreground colour fills the upper half of the cell, the background colour the lower half.  One column and half a
 * line make a square pixel, a terminal shows four times as many of them, and the text is 19.5 bytes per pixel.  For a screen of
 * `width` x `rows` owned rows, T = (rows + 1) / 2 text rows, in order:
 *   "\033[0;0H"                                                     6 bytes
 *   per text row i = 0 .. T-1:
 *     width cells "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm" E2 96 80   39 bytes each: RRR;GGG;BBB the emitter's (int)(c*255) of owned row
 *                                                                    2 i (the upper pixel), rrr;ggg;bbb those of owned row 2 i + 1 (the
 *                                                                    lower pixel), three zero-padded digits each (TRT.c:1134-1139)
 *     "\033[0m\n"                                                    5 bytes
 * When rows is odd the last text row's lower pixel is 000;000;000.  No NUL follows (the full text's are the reference's sizeof; this
 * format is the project's own).  Owned rows pair up in LOCAL order (local rows 2 i and 2 i + 1), as trt_render_device_ansi's shard
 * texts count their rows: a sharding host wants an even tile_rows, so that the pairs are neighbours in the frame.
 * csrc/trt_ansi_half.h is the format in code, trt_emitter_half_rgb8 (trt_host.h) its sequential statement on the host.  Checks, errors,
 * stream behaviour and the trt_kernel_times accounting of every entry are those of the _ansi entry it mirrors (the batch and host forms
 * stand with theirs below); capacities count bytes of text, to the byte.  None of them reads or changes the delta entries' shown
 * frame. */

/* Length of the half-block text: 6 + (39 * width + 5) * ((rows + 1) / 2), 0 unless both are positive. */
size_t trt_ansi_half_bytes(int width, int rows);
/* trt_render_device_ansi as the half-block text: trt_ansi_half_bytes(width, owned rows) bytes at d_text, any alignment, written by the
 * pass that forms the ordered mean -- a lane forms both pixels of its cell; neither doubles nor RGB8 bytes are written on the way, every
 * byte of the text is stored exactly once and none outside it (the reference-order kernel goes through a framebuffer and bytes of the
 * context's). */
int trt_render_device_ansi_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                                int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The formatting alone, of a frame that exists as RGB8 bytes in device memory (as trt_ansi_from_rgb8_device; e.g. what rank 0 of a
 * trt_dist_render_rgb8 gather holds): trt_ansi_half_bytes(width, rows) bytes at d_text, any alignment.  Asynchronous. */
int trt_ansi_half_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text);

/* ---- the kitty graphics-protocol image: true pixels, four bytes of text each ----------------------------------------------------
 * Both texts above paint a pixel with character cells, 25 and 19.5 bytes each.  Terminals that speak the kitty graphics protocol (kitty,
 * WezTerm, Ghostty, Konsole) take true pixels, as base64 of RGB bytes inside APC escape sequences: three bytes are exactly four base64
 * characters, so a pixel is one 32-bit word of text, a 1920 x 1080 frame 8.3 MB instead of 40 or 52, at full pixel resolution and
 * lossless.  For a screen of `width` x `rows` owned rows, P = width * rows pixels in LOCAL row order (for a shard, v is the owned rows),
 * K = ceil(P / 1024) chunks, in order:
 *   "\033[0;0H"                                                        6 bytes
 *   chunk 0:   "\033_Ga=T,f=24,i=1,p=1,q=2,C=1,s=WWWWW,v=RRRRR,m=M;"  48 bytes: WWWWW = width, RRRRR = rows, five zero-padded digits each
 *              the payload of chunk 0, then "\033\\"
 *   chunk c>0: "\033_Gm=0M;"                                           8 bytes
 *              the payload of chunk c, then "\033\\"
 * A payload holds the chunk's up to 1024 pixels, four characters each: RFC 4648 base64, standard alphabet, of the emitter's bytes R, G, B
 * ((int)(c*255), trt_render_device_rgb8's); 4096 characters are the protocol's limit per escape.  M is 1 in every chunk but the last, 0
 * in the last.  No '=', no newline, no NUL: 4 P + 10 K + 46 bytes.  a=T: transmit and display; f=24: RGB; i=1,p=1: image and placement
 * id, so that re-sending replaces the picture in place; q=2: the terminal answers nothing; C=1: the cursor stays.
 * NO TERMINAL HAS YET SHOWN THIS PICTURE: the key list is written from memory of the protocol, and the tests hold the text against a
 * structural reader, not a terminal.  csrc/trt_kitty.h is the format in code -- the 48-byte header ONE literal there --
 * trt_emitter_kitty_rgb8 (trt_host.h) its sequential statement on the host.  Limits: width <= 99999 and owned rows <= 99999; above them
 * the length is 0 and the entries return TRT_ERR_ARGUMENT.  Checks, errors, stream behaviour and the trt_kernel_times accounting of every
 * entry are otherwise those of the _ansi_half entry it mirrors; capacities count bytes of text, to the byte.  None of them reads or changes
 * the delta entries' shown frame.  There is no delta or animation form (a=f), no compression (o=z), no shared-memory transmission, no
 * refraction form and no tmux pass-through; of a trt_dist_render_rgb8 gather rank 0 formats the assembled bytes with
 * trt_kitty_from_rgb8_device. */

/* Length of the image text: 4 P + 10 ceil(P / 1024) + 46, P = width * rows; 0 unless both are positive and at most 99999. */
size_t trt_kitty_bytes(int width, int rows);
/* trt_render_device_ansi as the kitty image: trt_kitty_bytes(width, owned rows) bytes at d_text, any alignment, written by the pass that
 * forms the ordered mean -- a lane forms a pixel once and keeps its four characters in a register; neither doubles nor RGB8 bytes are
 * written on the way, every byte of the text is stored exactly once (d_text need not be initialised) and none outside it (the
 * reference-order kernel goes through a framebuffer and bytes of the context's). */
int trt_render_device_kitty(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                            int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The formatting alone, of a frame that exists as RGB8 bytes in device memory (as trt_ansi_from_rgb8_device; e.g. what rank 0 of a
 * trt_dist_render_rgb8 gather holds): trt_kitty_bytes(width, rows) bytes at d_text, any alignment.  Asynchronous. */
int trt_kitty_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text);

/* ---- the texts in the xterm 256-colour palette: for terminals without 24-bit colour ----------------------------------------------------
 * The two texts above colour their cells with "48;2;R;G;B", 24-bit SGR colour, and the kitty image needs a terminal that speaks that
 * protocol.  Terminal.app, older tmux and screen, PuTTY set-ups and many CI and serial consoles have only the palette of 256 colours:
 * "48;5;N".  Entries 0..15 of it are the user's to theme and are never produced; the 240 others are fixed numbers -- 16 + 36 i + 6 j + k
 * is the colour (L[i], L[j], L[k]), L = {0, 95, 135, 175, 215, 255}, and 232 + k is the grey 8 + 10 k, k = 0..23.  THE RULE: a pixel's
 * index is the entry, of these 240, with the least squared Euclidean distance in RGB bytes to the emitter's bytes of the pixel
 * ((int)(c*255), trt_render_device_rgb8's), ties to the lowest index.  trt_xterm256_index_search (trt_host.h) is that search;
 * csrc/trt_xterm256.h is the closed form of it that the device computes, equal to it on all 2^24 colours.  An index depends on the
 * pixel's three bytes alone: there is no dithering.
 *
 * The full 256-colour text.  For a screen of `width` x `rows` owned rows in LOCAL row order (for a shard, the owned rows), in order:
 *   "\033[0;0H"                                    6 bytes
 *   per owned row:  width cells "\033[48;5;NNNm  "  13 bytes each: NNN the pixel's index, three zero-padded digits
 *                   "\033[0m\n"                     5 bytes
 * 6 + (13 width + 5) rows bytes, no NUL.  It is not trt_ansi_bytes' text with other colours: rows end in a reset and no NULs follow.
 *
 * The half-block 256-colour text.  T = (rows + 1) / 2 text rows, in order:
 *   "\033[0;0H"                                                          6 bytes
 *   per text row t:  width cells "\033[38;5;UUU;48;5;LLLm" E2 96 80       23 bytes each: UUU the index of owned row 2 t, LLL that of owned
 *                                                                         row 2 t + 1; 016, black, behind the last row of an odd frame
 *                    "\033[0m\n"                                         5 bytes
 * 6 + (23 width + 5) T bytes, no NUL.  The terminal must be in a UTF-8 locale.
 *
 * csrc/trt_ansi256.h and csrc/trt_ansi256_half.h are the formats in code, trt_emitter_ansi256_rgb8 and trt_emitter_ansi256_half_rgb8
 * (trt_host.h) their sequential statements on the host.  Limits: those of the 24-bit texts (fewer than 2^31 - 1 pixels).  Checks,
 * TRT_ERR_*, stream behaviour and the trt_kernel_times accounting of every entry are those of the _ansi_half entry it mirrors;
 * capacities count bytes of text, to the byte.  These are the WHOLE texts: none of these entries reads or changes the delta entries'
 * shown frame; the delta forms of both, for the links where bytes per frame decide the frame rate, stand below the 24-bit delta texts
 * (trt_render_device_ansi256_delta, trt_render_device_ansi256_delta_half).  OUT OF SCOPE: no refraction form, no dithering and no
 * 16-colour text; of a trt_dist_render_rgb8 gather rank 0 formats the assembled bytes with the _from_rgb8_device entries.  No terminal was at hand to look at the picture: the tests hold the texts against
 * the sequential emitters and a structural reader. */

/* Lengths of the two texts: 6 + (13 width + 5) rows and 6 + (23 width + 5) ((rows + 1) / 2); 0 unless both arguments are positive. */
size_t trt_ansi256_bytes(int width, int rows);
size_t trt_ansi256_half_bytes(int width, int rows);
/* trt_render_device_ansi as the 256-colour text: trt_ansi256_bytes(width, owned rows) bytes at d_text, any alignment, written by the pass
 * that forms the ordered mean -- a lane forms a pixel once, maps it to the palette and keeps the index; neither doubles nor RGB8 bytes
 * are written on the way, every byte of the text is stored exactly once (d_text need not be initialised) and none outside it (the
 * reference-order kernel goes through a framebuffer and bytes of the context's). */
int trt_render_device_ansi256(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                              int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The same as the half-block 256-colour text: trt_ansi256_half_bytes(width, owned rows) bytes; a lane forms both pixels of a cell. */
int trt_render_device_ansi256_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                                   int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The formatting alone, of a frame that exists as RGB8 bytes in device memory (as trt_ansi_from_rgb8_device; e.g. what rank 0 of a
 * trt_dist_render_rgb8 gather holds): trt_ansi256_bytes / trt_ansi256_half_bytes(width, rows) bytes at d_text, any alignment.
 * Asynchronous. */
int trt_ansi256_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text);
int trt_ansi256_half_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text);
/* The palette map alone, trt_quantize_device's analogue: d_index[p] = the palette index 16..255 of the pixel d_rgb8[3 p ...], a paletted
 * frame at one byte a pixel, either pointer at any alignment.  Asynchronous on the context's stream; num_pixels 0 does nothing. */
int trt_xterm256_from_rgb8_device(trt_context *ctx, const void *d_rgb8, size_t num_pixels, void *d_index);

/* ---- the delta text: only the cells that changed --------------------------------------------------------------------------------
 * A terminal keeps what it was sent.  The text above repaints every cell of every frame, 25 bytes each; the DELTA text between the frame
 * the terminal shows and the next one holds, for every CHANGED cell (its three RGB8 bytes differ), rows ascending, left to right:
 *   "\033[RRRRR;CCCCCH"        14 bytes, where a run of consecutive changed cells of one row starts: RRRRR = owned row + 1,
 *                              CCCCC = 2 * column + 1 (a cell is two columns wide), five digits each, zero-padded
 *   "\033[48;2;RRR;GGG;BBBm"   19 bytes, where a run starts or the new colour differs from the new colour of the cell to the left
 *   two spaces
 *   "\033[0m"                   4 bytes, where the run ends (runs never continue into the next row)
 * and nothing for an unchanged cell: no prefix, no newline, no NUL; two equal frames give 0 bytes.  A text has at most
 * rows * (21 * width + 18) bytes (a run of L cells costs at most 18 + 21 L, and every further run of a row needs an unchanged cell
 * between), reached when every cell changed and no two horizontal neighbours share a colour.  Limits: width <= 49999, rows <= 99999
 * (five digits).  csrc/trt_ansi_delta.h is the format in code, trt_emitter_delta_rgb8 (trt_host.h) its sequential statement on the
 * host.  On the demo orbit at 60 frames per second the text is a third of the full one with the reference's smooth cubemap and a half to four
 * fifths with a noisy one (profiles/r11/a_delta.md).
 *
 * What a host of the render entries below must keep to:
 *   - it writes exactly the `bytes` bytes it is given, not the capacity;
 *   - a text it drops instead of writing is a frame the terminal never showed: call trt_ansi_delta_reset, the next text is a keyframe;
 *   - nothing else may be printed over the picture (a status line belongs on stderr or below the last row);
 *   - the refraction extension has no delta form; the batch entries have one (trt_render_device_batch_ansi_delta, below the batch
 *     entries); of a trt_dist_render_rgb8 gather rank 0 formats the assembled bytes with trt_ansi_delta_from_rgb8_device, several
 *     gathered frames at once with trt_ansi_delta_chain_from_rgb8_device;
 *   - the records here are of two-column cells of the full text in 24-bit colour.  The half-block text has a delta form of its own,
 *     below, and so have the two texts in the xterm 256-colour palette, below that: FOUR kinds.  A context keeps ONE shown frame and
 *     remembers which of the four it was sent as: a delta call is a keyframe unless the shown frame is of exactly this rowset AND this
 *     kind, so changing between any two kinds is a keyframe;
 *   - the sixel and kitty images and a 16-colour text have no delta form. */

/* Room for any text the delta entries write for a screen of `width` x `rows` owned rows: max(trt_ansi_bytes, rows * (21 * width + 18)),
 * the keyframe or the longest delta; 0 when either is not positive or above the limits. */
size_t trt_ansi_delta_capacity(int width, int rows);

/* The formatting alone, of two frames that exist as RGB8 bytes in device memory (rows x width x 3 each, any alignment): the delta text
 * that takes a terminal from d_shown_rgb8 to d_next_rgb8 at d_text (any alignment, need not be initialised), its length at *d_bytes --
 * a DEVICE address, 8-byte aligned.  Three kernels in stream order (csrc/trt_ansi_delta.hpp): record lengths summed per tile of 1024
 * cells, one workgroup's exclusive scan of the sums, the records stored at their offsets; every byte below the length is stored once,
 * none at or behind it.  It neither reads nor changes the context's shown frame.  capacity_bytes >= trt_ansi_delta_capacity(width,
 * rows), else TRT_ERR_CAPACITY; NULL or a size above the limits: TRT_ERR_ARGUMENT.  Asynchronous on the context's stream. */
int trt_ansi_delta_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows,
                                    void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);

/* trt_render_device as the delta text against the context's SHOWN frame: the RGB8 bytes of the frame this entry (or the host entry
 * below) rendered last, kept in one of two buffers of the context that swap per call.  The new frame's bytes are written by the RGB8
 * form of the ordered-mean pass (trt_render_device_rgb8; the reference-order kernel goes through trt_quantize_device's kernel), then
 * compared with the shown ones by the three kernels above.  When the context has no shown frame for exactly this rowset -- the first
 * call, another trt_rowset, after trt_ansi_delta_reset, after a call that failed once it had begun to enqueue, or after a call of
 * the half-block kind (trt_render_device_ansi_delta_half below), whose shown frame was sent as another text -- the call is a
 * KEYFRAME: d_text is byte for byte trt_render_device_ansi's text and *d_bytes = trt_ansi_bytes(width, owned rows).  Either way the new
 * frame becomes the shown one.  Every other render entry and trt_set_scene leave the shown frame alone: what the terminal shows did
 * not change.  Rows count from the shard's first owned row, as in trt_render_device_ansi's shard texts.
 * Errors, before anything is enqueued (the shown frame is kept): NULL, an invalid rowset, no owned row, a size above the limits ->
 * TRT_ERR_ARGUMENT; no scene -> TRT_ERR_NO_SCENE; capacity_bytes < trt_ansi_delta_capacity(width, owned rows) -> TRT_ERR_CAPACITY.
 * Asynchronous on the context's stream; d_bytes as above.  One entry of trt_kernel_times (the render and the ordered mean; the text
 * kernels follow it). */
int trt_render_device_ansi_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                 void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* The same into HOST memory, synchronous: the length is read back, then exactly *bytes bytes cross PCIe through the pinned staging --
 * two small transfers instead of one large one.  capacity_bytes counts the bytes at text, checked as above. */
int trt_render_host_ansi_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                               char *text, size_t capacity_bytes, size_t *bytes);
/* Forget the shown frame: the next delta call, of any of the four kinds, returns a keyframe.  For a host that dropped a text, cleared its
 * terminal or printed over the picture. */
int trt_ansi_delta_reset(trt_context *ctx);

/* ---- the delta text in half-block cells ------------------------------------------------------------------------------------------
 * The delta text of a terminal that shows the HALF-BLOCK text: the cells are that text's, T = (rows + 1) / 2 text rows of `width`
 * one-column cells, cell (t, c) with the upper pixel of owned row 2 t and the lower pixel of owned row 2 t + 1 (000;000;000 behind an
 * odd frame's last row, in both frames; never read from memory).  A cell is CHANGED when either pixel differs.  For every changed
 * cell, text rows ascending, left to right:
 *   "\033[RRRRR;CCCCCH"        14 bytes, where a run of consecutive changed cells of one text row starts: RRRRR = t + 1, CCCCC = c + 1
 *   the colours, against the new colours of the cell to the left, which the run has just painted:
 *     "\033[38;2;RRR;GGG;BBB;48;2;rrr;ggg;bbbm"   36 bytes, where a run starts or BOTH differ
 *     "\033[38;2;RRR;GGG;BBBm"                    19 bytes, where only the upper colour differs
 *     "\033[48;2;rrr;ggg;bbbm"                    19 bytes, where only the lower colour differs
 *     nothing                                     where neither differs
 *   E2 96 80                    3 bytes, the glyph U+2580
 *   "\033[0m"                   4 bytes, where the run ends
 * so a record has 3, 7, 22, 26, 39, 43, 53 or 57 bytes; no prefix, no newline, no NUL; equal frames give 0 bytes.  A text has at most
 * T * (39 * width + 18) bytes, reached when every cell changed and both colours differ from the left neighbour's everywhere.  Limits:
 * width <= 99999, T <= 99999 (rows <= 199998).  csrc/trt_ansi_delta_half.h is the format in code, trt_emitter_delta_half_rgb8
 * (trt_host.h) its sequential statement on the host; the measured bytes and times are in profiles/r15/a_delta_half.md.  The rules for
 * the host are those of the delta text above.  The batch form stands with the full kind's, below the batch entries; there is no
 * refraction form. */

/* Room for any text the half-block delta entries write: max(trt_ansi_half_bytes, ((rows + 1) / 2) * (39 * width + 18)), the keyframe or
 * the longest delta; 0 when either size is not positive or above the limits. */
size_t trt_ansi_delta_half_capacity(int width, int rows);

/* trt_ansi_delta_from_rgb8_device for half-block cells: the text that takes a terminal from the half-block text of d_shown_rgb8 to that
 * of d_next_rgb8 (rows x width x 3 bytes each, any alignment; nothing behind an odd frame's last row is read).  Three kernels in stream
 * order (csrc/trt_ansi_delta.hpp; the scan of the tiles' sums is the delta text's own).  It neither reads nor changes the context's
 * shown frame; it is what rank 0 applies to a trt_dist_render_rgb8 gather.  capacity_bytes >= trt_ansi_delta_half_capacity(width, rows),
 * else TRT_ERR_CAPACITY; NULL or a size above the limits: TRT_ERR_ARGUMENT.  Asynchronous on the context's stream. */
int trt_ansi_delta_half_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows,
                                         void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);

/* trt_render_device_ansi_delta in half-block cells, on the same shown frame.  A context keeps ONE shown frame and remembers which
 * text it was sent as: this call is a KEYFRAME when there is no shown frame for exactly this rowset AND this kind -- the first call,
 * another trt_rowset, after trt_ansi_delta_reset, after a call that failed once it had begun to enqueue, or after a
 * trt_render_*_ansi_delta call of the full-text kind (which in turn is a keyframe after one of these: a terminal that shows two-column
 * cells cannot be patched with one-column records).  The keyframe is byte for byte trt_render_device_ansi_half's text and *d_bytes =
 * trt_ansi_half_bytes(width, owned rows).  Errors as trt_render_device_ansi_delta, with trt_ansi_delta_half_capacity and this kind's
 * limits. */
int trt_render_device_ansi_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                      void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* The same into HOST memory, synchronous: the 8-byte length is read back, then exactly *bytes bytes cross PCIe. */
int trt_render_host_ansi_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                    char *text, size_t capacity_bytes, size_t *bytes);

/* ---- the delta texts in the xterm 256-colour palette --------------------------------------------------------------------------------
 * The delta texts of a terminal that shows the 256-COLOUR texts (trt_render_device_ansi256, trt_render_device_ansi256_half): the links
 * that have only the palette -- ssh, an old tmux, a serial or CI console -- are those where bytes per frame decide the frame rate.  The
 * frames are the same RGB8 bytes; a pixel's INDEX is its palette entry 16..255 (the rule above the 256-colour texts).  A cell is CHANGED
 * when an INDEX differs, not when a byte does: a cell whose bytes move inside one palette entry has no record, so the text has at most
 * as many records as the 24-bit delta of the same two frames, and each is shorter.  Runs, record order and the cursor are those of the
 * 24-bit kind of the same cells; "the same as the left neighbour's" compares NEW INDICES.
 *
 * Full cells (two columns wide), a record:
 *   "[RRRRR;CCCCCH"        14 bytes, where a run starts: RRRRR = owned row + 1, CCCCC = 2 * column + 1
 *   "[48;5;NNNm"           11 bytes, where a run starts or the new index differs from the left neighbour's new index
 *   two spaces
 *   "[0m"                   4 bytes, where the run ends
 * 2, 6, 13, 17, 27 or 31 bytes.  A text has at most rows * (13 * width + 13 + 5 * ((width + 1) / 2)) bytes: here a run's fixed cost (18)
 * exceeds a cell's (13), so MORE runs cost more -- with k runs a row holds at most width - k + 1 changed cells, 18 k + 13 (width - k + 1)
 * bytes, which grows up to k = (width + 1) / 2 -- reached by changed and unchanged cells in turn.  Limits: width <= 49999, rows <= 99999.
 *
 * Half-block cells (T = (rows + 1) / 2 text rows, upper pixel owned row 2 t, lower pixel owned row 2 t + 1; index 016 behind an odd
 * frame's last row in both frames, never read from memory), a record:
 *   "[RRRRR;CCCCCH"        14 bytes, where a run starts: RRRRR = t + 1, CCCCC = c + 1
 *   "[38;5;UUU;48;5;LLLm"  20 bytes, where a run starts or BOTH indices differ from the left neighbour's
 *   "[38;5;UUUm"           11 bytes, where only the upper index differs
 *   "[48;5;LLLm"           11 bytes, where only the lower index differs; nothing where neither differs
 *   E2 96 80                    3 bytes, the glyph U+2580
 *   "[0m"                   4 bytes, where the run ends
 * 3, 7, 14, 18, 23, 27, 37 or 41 bytes.  A text has at most T * (23 * width + 18) bytes (one run is worst, as in the 24-bit kind).
 * Limits: width <= 99999, T <= 99999.
 *
 * csrc/trt_ansi256_delta.h and csrc/trt_ansi256_delta_half.h are the formats in code, trt_emitter_delta256_rgb8 and
 * trt_emitter_delta256_half_rgb8 (trt_host.h) their sequential statements on the host; the measured bytes and times are in
 * profiles/r26/a_delta256.md.  Every entry below mirrors the 24-bit delta entry of the same name without "256": semantics, errors,
 * stream behaviour and trt_kernel_times accounting are that entry's, the capacity, the limits and the keyframe this kind's.  The rules
 * for the host are those of the delta text above.  OUT OF SCOPE: no refraction form, no sixel, kitty or 16-colour delta.
 * The entries of this family are declared `extern int`, which says what `int` says: the table of stream-order scenarios that
 * tests/test_ansi256_stream_order.py holds against the `int trt_...256...` declarations of this header is that of the WHOLE 256-colour
 * texts; this family's asynchronous entries have their scenarios, and the check that none lacks one, in
 * tests/test_ansi256_delta_stream_order.py. */

/* Room for any text the 256-colour delta entries write: the larger of the whole text (trt_ansi256_bytes, trt_ansi256_half_bytes) -- the
 * keyframe -- and the bound above; 0 when either size is not positive or above the limits. */
size_t trt_ansi256_delta_capacity(int width, int rows);
size_t trt_ansi256_delta_half_capacity(int width, int rows);

/* trt_ansi_delta_from_rgb8_device and trt_ansi_delta_half_from_rgb8_device in the palette: the frames are RGB8 bytes (what a
 * trt_dist_render_rgb8 gather holds), which the kernels map to indices as they load them; no paletted copy of a frame is made.  They
 * neither read nor change the context's shown frame.  capacity_bytes >= the kind's capacity, else TRT_ERR_CAPACITY. */
extern int trt_ansi256_delta_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows,
                                              void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
extern int trt_ansi256_delta_half_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_next_rgb8, int width, int rows,
                                                   void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);

/* trt_render_device_ansi_delta and trt_render_device_ansi_delta_half in the palette, on the same ONE shown frame: a KEYFRAME unless the
 * context has a shown frame for exactly this rowset AND this kind of the four.  The keyframe is byte for byte
 * trt_render_device_ansi256's (or trt_render_device_ansi256_half's) text, *d_bytes its length. */
extern int trt_render_device_ansi256_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                           void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
extern int trt_render_device_ansi256_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                                                int rays_per_pixel, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* The same into HOST memory, synchronous: the 8-byte length is read back, then exactly *bytes bytes cross PCIe. */
extern int trt_render_host_ansi256_delta(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                         char *text, size_t capacity_bytes, size_t *bytes);
extern int trt_render_host_ansi256_delta_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                              char *text, size_t capacity_bytes, size_t *bytes);

/* ---- the DEC sixel image: true pixels for the terminals that take sixel and nothing else -----------------------------------------------
 * The kitty image above reaches kitty, WezTerm, Ghostty and Konsole.  xterm, foot, mlterm, Windows Terminal, VS Code's terminal, contour
 * and tmux built with sixel take SIXEL: a picture in bands of six pixel rows, a band drawn one colour register at a time, a data
 * character six pixels of one column.  For a screen of `width` x `rows` owned rows in LOCAL row order, in order:
 *   "\033[0;0H"                       6 bytes   cursor home
 *   "\033P0;1;0q"                     8 bytes   DCS, P2 = 1: a 0 bit leaves its pixel alone
 *   "\"1;1;WWWWW;RRRRR"              16 bytes   raster attributes: width and rows, five zero-padded digits each
 *   240 x "#NNN;2;PPP;PPP;PPP"     4320 bytes   colour register NNN = 016..255, ascending: the xterm palette's entry NNN (the 6 x 6 x 6 cube
 *                                               and the grey ramp, trt_host.h) in RGB per cent, PPP = (100 v + 127) / 255 in integers
 *   per band b of six pixel rows (the last has fewer), per palette index n, ASCENDING, that a pixel of the band has
 *   (trt_xterm256_index of its emitter bytes), a colour row:
 *     "#NNN"                          4 bytes
 *     width data characters           63 + the sum over j of (the pixel of row 6 b + j in this column has index n) << j
 *     T - 1 times "$", one more byte  "-" behind the LAST colour of every band but the last band, "$" everywhere else
 *   "\033\\"                          2 bytes
 * T = 1 + ((-(width + 1)) mod 4), so a colour row is L = 4 + width + T bytes, a multiple of 4 (a repeated "$" is a repeated graphics
 * carriage return and changes nothing).  The text has 4352 + L * (the colour rows of all bands) bytes -- its length DEPENDS ON THE
 * PICTURE, so every entry reports it, as the delta entries do.  No NUL, no newline.
 * NO TERMINAL HAS SHOWN THIS PICTURE: the format is written from memory of DEC's description, and the tests hold the text against a
 * structural reader (tests/sixel_support.py), not a terminal.  Registers up to 255 need a terminal with 256 colour registers: xterm as a
 * VT340 defaults to 16 and needs `numColorRegisters: 256`.  A per-cent palette cannot say 95 or 135 exactly, so the colours are within
 * 1/100 of the xterm palette's.  csrc/trt_sixel.h is the format in code, trt_emitter_sixel_rgb8 (trt_host.h) its sequential statement on
 * the host.  Limits: width <= 99999 and owned rows <= 99999; above them the capacity is 0 and the entries return TRT_ERR_ARGUMENT.
 * There are no "!" run-length repeats, no dithering, no palette other than the 240 fixed entries, no delta form, no batch forms, no
 * refraction form and no tmux pass-through; of a trt_dist_render_rgb8 gather rank 0 formats the assembled bytes with
 * trt_sixel_from_rgb8_device. */

/* Room for any image of the size: 4352 + L * the sum over the bands of min(240, width * the band's rows); 0 unless both sizes are positive
 * and at most 99999. */
size_t trt_sixel_capacity(int width, int rows);

/* The formatting alone, of a frame that exists as RGB8 bytes in device memory (rows x width x 3, any alignment): the image at d_text (any
 * alignment, need not be initialised), its length at *d_bytes -- a DEVICE address, 8-byte aligned.  Three kernels in stream order
 * (csrc/trt_sixel.hpp), no atomic on device memory and no workgroup that waits for another: a workgroup per band ORs its pixels' indices
 * into a 240-bit mask; one workgroup scans the bands' colour counts into offsets, stores the length and writes the 4350 bytes in front of
 * the first colour row and the 2 behind the last; a thread per four adjacent columns of a band keeps their 6 x 4 indices in registers,
 * walks the band's mask and stores an aligned 32-bit word per colour.  Every byte below the length is stored once, none at or behind it.
 * It neither reads nor changes the context's shown frame.  capacity_bytes >= trt_sixel_capacity(width, rows), else TRT_ERR_CAPACITY; NULL
 * or a size that is not positive or above the limits: TRT_ERR_ARGUMENT.  Asynchronous on the context's stream. */
int trt_sixel_from_rgb8_device(trt_context *ctx, const void *d_rgb8, int width, int rows, void *d_text, size_t capacity_bytes,
                               unsigned long long *d_bytes);
/* trt_render_device as the sixel image: the frame's bytes are written by the RGB8 form of the ordered-mean pass into a buffer of the
 * context's that is NOT one of the delta entries' shown pair (the reference-order kernel goes through trt_quantize_device's kernel), then
 * formatted by the three kernels above.  The delta entries' shown frame is neither read nor changed.  For a shard the raster's rows are
 * the owned rows, in local order.  Errors, before anything is enqueued: NULL, an invalid rowset, a size above the limits ->
 * TRT_ERR_ARGUMENT; no scene -> TRT_ERR_NO_SCENE; capacity_bytes < trt_sixel_capacity(width, owned rows) -> TRT_ERR_CAPACITY.
 * Asynchronous on the context's stream; d_bytes as above.  One entry of trt_kernel_times (the render and the ordered mean; the image's
 * kernels follow it). */
int trt_render_device_sixel(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                            void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* The same into HOST memory, synchronous: the length is read back, then exactly *bytes bytes cross PCIe through the pinned staging.
 * capacity_bytes counts the bytes at text, checked as above. */
int trt_render_host_sixel(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                          char *text, size_t capacity_bytes, size_t *bytes);

/* Same as trt_render_device but into HOST memory (synchronous; pinned staging inside). */
int trt_render_host(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit,
                    int rays_per_pixel, Vector *pixels);

/* trt_render_device_rgb8 into HOST memory: the emitter's (int)(c*255), 3 bytes per pixel (synchronous; pinned staging inside). */
int trt_render_host_rgb8(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                         unsigned char *rgb);

/* trt_render_device_ansi into HOST memory: trt_ansi_bytes(width, owned rows) bytes (synchronous; one copy-out through pinned staging). */
int trt_render_host_ansi(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                         char *text);

/* trt_render_device_ansi_half into HOST memory: trt_ansi_half_bytes(width, owned rows) bytes (synchronous; one copy-out through pinned
 * staging). */
int trt_render_host_ansi_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                              char *text);

/* trt_render_device_kitty into HOST memory: trt_kitty_bytes(width, owned rows) bytes (synchronous; one copy-out through pinned staging). */
int trt_render_host_kitty(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                          char *text);

/* trt_render_device_ansi256 and trt_render_device_ansi256_half into HOST memory: trt_ansi256_bytes / trt_ansi256_half_bytes(width, owned
 * rows) bytes (synchronous; one copy-out through pinned staging). */
int trt_render_host_ansi256(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                            char *text);
int trt_render_host_ansi256_half(trt_context *ctx, const Camera *camera, const trt_rowset *rows, int bounce_limit, int rays_per_pixel,
                                 char *text);

/* Several cameras of the current scene in one call: an orbit, a replay, a stereo pair, the faces of an environment probe. */
#define TRT_BATCH_MAX 8 /* = the eye-table slots a scene's tables have */

/* n cameras, one call, one context, one stream.  Frame b goes to d_pixels + b * (owned rows * width) Vectors, each frame in
 * the layout trt_render_device writes; every frame is bit-identical to what trt_render_device gives for that camera.
 * All cameras must have the same screen_width / screen_height / screen_distance (main() moves only camera.frame,
 * TRT.c:1327-1336); 1 <= n <= TRT_BATCH_MAX.  Asynchronous on the context's stream.
 * Where the production kernel has a form for it (image in LDS, no counters, no refraction, 256-thread or decoupled
 * workgroups) ONE persistent launch works through the samples of all n frames, frame b's tail filled by frame b + 1's
 * head; a batch whose larger LDS image (28 doubles per extra camera) would cost a resident workgroup is split into the
 * largest batches that do not; everything else is served one launch per camera on the same stream (trt_batch_info).
 * Errors, before anything is enqueued: NULL, n out of range, cameras whose screens differ, an invalid rowset, n frames
 * of 2^31 samples or more -> TRT_ERR_ARGUMENT; no scene -> TRT_ERR_NO_SCENE; a buffer too small for n frames ->
 * TRT_ERR_CAPACITY; n > 1 on a context whose tables are shared (trt_share_scene, either side: the eye slots a batch
 * would build its tables in are the sharers') -> TRT_ERR_CAPACITY.  The sample scratch is n x 24 B x rays_per_pixel per
 * pixel.  trt_kernel_times / trt_render_kernel_times count a batch as ONE entry (events around the whole batch). */
int trt_render_device_batch(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                            int rays_per_pixel, void *d_pixels, size_t capacity_bytes);
/* The same into HOST memory: pixels[b * owned rows * width ...] (synchronous; one copy-out through pinned staging). */
int trt_render_host_batch(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                          int rays_per_pixel, Vector *pixels);
/* trt_render_device_batch as the emitter's bytes (trt_render_device_rgb8): frame b at d_rgb8 + b * owned rows * width * 3, which
 * need not be aligned to anything; every frame is byte for byte what trt_render_device_rgb8 gives for that camera.  One launch, a
 * split for LDS or one launch per camera exactly as trt_render_device_batch decides (trt_batch_info); the same errors, the capacity
 * counted in bytes of RGB8 for n frames. */
int trt_render_device_batch_rgb8(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                 int rays_per_pixel, void *d_rgb8, size_t capacity_bytes);
/* The same into HOST memory: rgb[b * owned rows * width * 3 ...] (synchronous; one copy-out through pinned staging). */
int trt_render_host_batch_rgb8(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                               int rays_per_pixel, unsigned char *rgb);
/* trt_render_device_batch as the terminal's text (trt_render_device_ansi): frame b at d_text + b * trt_ansi_bytes(width, owned rows),
 * which is aligned to nothing in general (the text of 160 x 48 is 192057 bytes long); launches, splits and trt_batch_info exactly as
 * trt_render_device_batch decides them; the same errors, the capacity counted in bytes of text for n frames. */
int trt_render_device_batch_ansi(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                 int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The same into HOST memory: text[b * trt_ansi_bytes(width, owned rows) ...] (synchronous; one copy-out through pinned staging). */
int trt_render_host_batch_ansi(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                               int rays_per_pixel, char *text);
/* trt_render_device_batch as the half-block text (trt_render_device_ansi_half): frame b at d_text + b * trt_ansi_half_bytes(width, owned
 * rows), aligned to nothing in general; launches, splits, trt_batch_info and errors as trt_render_device_batch_ansi, the capacity
 * counted in bytes of text for n frames. */
int trt_render_device_batch_ansi_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                      int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The same into HOST memory: text[b * trt_ansi_half_bytes(width, owned rows) ...] (synchronous; one copy-out through pinned staging). */
int trt_render_host_batch_ansi_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                    int rays_per_pixel, char *text);

/* trt_render_device_batch as the kitty image (trt_render_device_kitty): frame b at d_text + b * trt_kitty_bytes(width, owned rows), aligned
 * to nothing in general; launches, splits, trt_batch_info and errors as trt_render_device_batch_ansi, the capacity counted in bytes of
 * text for n frames. */
int trt_render_device_batch_kitty(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                  int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The same into HOST memory: text[b * trt_kitty_bytes(width, owned rows) ...] (synchronous; one copy-out through pinned staging). */
int trt_render_host_batch_kitty(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                int rays_per_pixel, char *text);

/* trt_render_device_batch as the 256-colour texts (trt_render_device_ansi256, trt_render_device_ansi256_half): frame b at d_text + b *
 * trt_ansi256_bytes / trt_ansi256_half_bytes(width, owned rows), aligned to nothing in general; launches, splits, trt_batch_info and
 * errors as trt_render_device_batch_ansi, the capacity counted in bytes of text for n frames. */
int trt_render_device_batch_ansi256(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                    int rays_per_pixel, void *d_text, size_t capacity_bytes);
int trt_render_device_batch_ansi256_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                         int rays_per_pixel, void *d_text, size_t capacity_bytes);
/* The same into HOST memory: text[b * trt_ansi256_bytes / trt_ansi256_half_bytes(width, owned rows) ...] (synchronous; one copy-out
 * through pinned staging). */
int trt_render_host_batch_ansi256(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                  int rays_per_pixel, char *text);
int trt_render_host_batch_ansi256_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                       int rays_per_pixel, char *text);

/* ---- delta texts for a batch: n texts back to back, one prefix sum over all frames --------------------------------------------------
 * A CHAIN is a shown frame and n frames of RGB8 bytes (rows x width x 3 each), 1 <= n <= TRT_BATCH_MAX.  Text b takes a terminal from
 * frame b - 1 to frame b, for b = 0 from the shown frame; each is byte for byte the delta text of its two frames (above).  The texts
 * stand back to back: text b starts at the sum of the lengths before it, a text of 0 bytes where the next one starts.  The per-frame
 * cost of the one-frame entries -- three launches, two round trips -- is paid once per chain (csrc/trt_ansi_delta_chain.h states the
 * chain in code; profiles/r18/a_delta_batch.md has the measurement). */

/* The formatting alone: the shown frame at d_shown_rgb8, the n frames back to back at d_frames_rgb8 (frame stride rows * width * 3, no
 * padding, any alignment), the n texts back to back at d_text (any alignment), their n lengths at d_bytes[0..n) -- a DEVICE address,
 * 8-byte aligned.  THREE launches whatever n is: measure and write over the tiles of all n pairs of frames, one workgroup's scan
 * over all their sums between them.  Every byte below the sum of the lengths is stored once, none at or behind it.  It neither reads nor
 * changes the context's shown frame; it is what rank 0 applies to several gathered trt_dist_render_rgb8 frames.  capacity_bytes >=
 * n * trt_ansi_delta_capacity(width, rows), else TRT_ERR_CAPACITY; NULL, n out of range or a size above the limits: TRT_ERR_ARGUMENT.
 * Asynchronous on the context's stream. */
int trt_ansi_delta_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                          void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* The same in half-block cells; capacity_bytes >= n * trt_ansi_delta_half_capacity(width, rows).  Behind an odd frame's last pixel row
 * lies the next frame of the chain: it is not read as a lower row, the last text row's lower halves are black in every text. */
int trt_ansi_delta_half_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                               void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);

/* trt_render_device_batch_rgb8 into a buffer of the context -- one launch, a split for LDS or one launch per camera, as it decides;
 * trt_batch_info reports the batch, trt_kernel_times counts one entry -- and the n frames' delta texts as one chain.  Text 0 is against
 * the context's SHOWN frame, which the context has for exactly this rowset and this kind under the rules of
 * trt_render_device_ansi_delta; if it has none, text 0 is the KEYFRAME, byte for byte trt_render_device_ansi's text, d_bytes[0] its
 * length, and the chain of the other frames starts behind it.  Texts 1..n-1 are against the previous frame of the batch.  Afterwards
 * frame n - 1 is the shown frame, of this rowset and this kind (where it was rendered: no frame is copied): a later trt_render_*_ansi_delta call
 * continues from it, and a batch continues from theirs.
 * Errors before anything is enqueued, the shown frame kept: those of trt_render_device_batch_rgb8 (n > 1 on shared tables:
 * TRT_ERR_CAPACITY) and of trt_render_device_ansi_delta, with capacity_bytes >= n * trt_ansi_delta_capacity(width, owned rows).  A
 * failure behind that point forgets the shown frame.  Asynchronous on the context's stream; d_bytes: n lengths at a DEVICE address,
 * 8-byte aligned. */
int trt_render_device_batch_ansi_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                       int rays_per_pixel, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* The same in half-block cells: the keyframe is trt_render_device_ansi_half's text, capacity_bytes >= n *
 * trt_ansi_delta_half_capacity(width, owned rows). */
int trt_render_device_batch_ansi_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                            int rays_per_pixel, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
/* Into HOST memory, synchronous: one transfer of the n lengths, then one of exactly their sum through the pinned staging.  bytes[b] is
 * text b's length, the texts stand back to back at text; capacity_bytes counts the bytes at text, checked as above.  If a copy fails
 * the shown frame is forgotten. */
int trt_render_host_batch_ansi_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                     int rays_per_pixel, char *text, size_t capacity_bytes, size_t *bytes);
int trt_render_host_batch_ansi_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                          int rays_per_pixel, char *text, size_t capacity_bytes, size_t *bytes);

/* The six entries above in the xterm 256-colour palette (the delta texts in the palette, above): each is the entry of the same name
 * without "256" -- launches, texts back to back, lengths, trt_batch_info, errors, stream behaviour -- with this kind's cells, capacity
 * (n * trt_ansi256_delta_capacity / trt_ansi256_delta_half_capacity) and limits, and with trt_render_device_ansi256's or
 * trt_render_device_ansi256_half's text as the keyframe.  Two frames of a chain that map to the same indices give a text of 0 bytes. */
extern int trt_ansi256_delta_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width, int rows,
                                                    void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
extern int trt_ansi256_delta_half_chain_from_rgb8_device(trt_context *ctx, const void *d_shown_rgb8, const void *d_frames_rgb8, int n, int width,
                                                         int rows, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
extern int trt_render_device_batch_ansi256_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                                 int rays_per_pixel, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
extern int trt_render_device_batch_ansi256_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                                      int rays_per_pixel, void *d_text, size_t capacity_bytes, unsigned long long *d_bytes);
extern int trt_render_host_batch_ansi256_delta(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                               int rays_per_pixel, char *text, size_t capacity_bytes, size_t *bytes);
extern int trt_render_host_batch_ansi256_delta_half(trt_context *ctx, const Camera *cameras, int n, const trt_rowset *rows, int bounce_limit,
                                                    int rays_per_pixel, char *text, size_t capacity_bytes, size_t *bytes);

/* The most recent batch call of this context: its frames, and how many render-kernel launches served them
 * (1 = one launch over all frames; n = one launch per camera; between: the batch was split for LDS). */
int trt_batch_info(trt_context *ctx, int *frames, int *render_launches);

int trt_synchronize(trt_context *ctx);

/* HIP-event durations (ms) of the most recent render-kernel launches on this context, newest
 * last; returns how many were written (<= max).  Synchronises the stream. */
int trt_kernel_times(trt_context *ctx, float *ms, int max);
/* The same launches split at the HIP event recorded between the two kernels of a frame: the render kernel's own
 * duration and that of the ordered mean over a pixel's samples (TRT.c:1063-1065); reduce_ms may be NULL. */
int trt_render_kernel_times(trt_context *ctx, float *render_ms, float *reduce_ms, int max);

/* Kernel selection: 0 = production kernel (persistent waves, mode-synchronous rounds over single samples, then the
 * ordered mean per pixel); 1 = reference-order kernel (one lane per pixel, loops exactly as TRT.c:966-1069, every
 * sphere tested, no culling): an independent implementation kept as the on-device parity anchor.  Both are HIP; there
 * is no CPU path. */
int trt_set_kernel(trt_context *ctx, int which);

/* Light-space candidate masks of the production kernel (csrc/trt_lightgrid.h): a shadow ray reads the spheres it can
 * touch from a table of its light -- a directional_cells^2 grid across a directional light's direction, a cube map
 * of 6 * point_cells^2 direction cells about a point light -- instead of sweeping all spheres.  Built on the host
 * whenever the spheres or the lights change.  0, 0 turns the tables off (every shadow ray sweeps); results are
 * bit-identical either way.  Defaults: 128 and 64; environment TRT_LIGHTGRID="d,p" overrides the defaults. */
int trt_set_light_grids(trt_context *ctx, int directional_cells, int point_cells);
/* The tables' third coordinate (csrc/trt_lightgrid.h (5)): `directional_slabs` slabs of depth along a directional light's
 * direction, `point_shells` shells of distance from a point light (1..64 each); a cell then lists only the spheres that can lie
 * between an origin of its slab and the light -- about half the column in a dense scene.  1, 1: the two-parameter tables of
 * rounds 1-3.  Defaults 16 and 16; TRT_LIGHTGRID="d,p,slabs,shells" sets all four.  Frames are bit-identical for every value. */
int trt_set_light_slabs(trt_context *ctx, int directional_slabs, int point_shells);

/* Candidate tables of the PATH rays (csrc/trt_raygrid.h): path rays come in families that pass (nearly) through one point --
 * the eye, its mirror image in the ground, a sphere, a sphere's mirror image -- and each family has a cube map of
 * 6 * cells^2 direction cells listing the spheres its rays can touch; a path ray reads ONE cell instead of sweeping all
 * spheres (TRT.c:805-828 tests every sphere).  eye_cells: per face side for the two families of the eye (rebuilt on the GPU
 * when the eye moves), sphere_cells: for the 2N families of the spheres (rebuilt when spheres or ground change).
 * 0, 0 turns them off (every path ray sweeps); frames are bit-identical either way.  Defaults 64 and 32; environment
 * TRT_PATHGRID="e,s" overrides the defaults.  Scenes with more than 256 spheres render without any candidate table. */
int trt_set_path_grids(trt_context *ctx, int eye_cells, int sphere_cells);
/* Sub-families of the spheres (csrc/trt_raygrid.h).  "Every ray that starts anywhere on sphere i" is a fat family: in a dense
 * scene (256 spheres) its direction cells list 6.5 candidates per path ray for 1.1 exact hits.  With m > 0 the surface of
 * every sphere is cut into 6 m^2 patches (a cube map of the direction centre -> origin) and each patch -- and its mirror image
 * in the ground -- gets its own family and table: apex under the middle of the patch, membership radius 0.82 / 0.52 / 0.44 /
 * 0.33 of the sphere's for m = 1..4, hence narrower cones and shorter lists (3.6 candidates at m = 2) for 6 m^2 times the
 * table memory (sphere_cells = 32, 256 spheres: 25 MB at m = 0, 604 MB at m = 2).  The membership of every ray in the family
 * it is looked up in is still checked in FP64 per ray; frames are bit-identical for every m.  m = -1 (default): 2 for scenes of
 * 128 spheres or more, else 0.  Environment TRT_PATHGRID="e,s,m" sets all three defaults. */
int trt_set_path_patches(trt_context *ctx, int m);
/* m and the patches per sphere (1, or 6 m^2) of the tables the current scene renders with; 0, 0 when the tables are off */
int trt_get_path_patches(trt_context *ctx, int *m, int *patches_per_sphere);
/* Scenes with fewer than `min_spheres` spheres keep the sweep for their path rays: below about a dozen spheres 9 VALU per
 * sphere are cheaper than a look-up with its membership test (default 12; 0 = tables for every scene). */
int trt_set_path_grids_min_spheres(trt_context *ctx, int min_spheres);

/* Shading decoupled from the lane that owns the sample (render_rounds_kernel<.., .., true>): the hits of a
 * wave become tasks in a ring in LDS and are shaded 64 at a time, whichever lanes they came from, so that the shadow rays run
 * with ~96 % of the lanes busy instead of ~61 % (the share of path rays that hit something).  The ring costs about what one
 * light's idle lanes cost, and its 1024-thread workgroups suit large launches: mode -1 (default) uses it for scenes with two
 * lights or more and launches of 16 M samples or more (a 1080p frame at 10 rays per pixel is 20.7 M; row shards of 1/2 and
 * less stay on the plain rounds), when the rings fit in LDS beside the scene without costing a resident wave (up to ~100
 * spheres); 0: never; 1: whenever the rings fit.  Frames are bit-identical in every mode.  Environment TRT_COMPACTION=-1|0|1
 * sets the default of new contexts. */
int trt_set_compaction(trt_context *ctx, int mode);
/* Which form a frame of the current scene and of the most recent launch's size runs (a whole large frame before the first
 * launch): *decoupled 1 / 0, and the threads of a workgroup (1024 / 256). */
int trt_render_variant(trt_context *ctx, int *decoupled, int *workgroup_threads);

/* EXTENSION, PARITY UNPINNED.  The reference has no refraction (Material is {color, reflectivity, specularity},
 * TRT.c:114-119, and only the near root of a sphere is ever used, TRT.c:657); BASELINE config 3 names "refractive
 * materials" all the same.  ior[i] > 0 makes sphere i of the current scene a refractor with that index of refraction
 * (relative to the outside), 0 leaves it the reference's opaque sphere; the Material layout is untouched.  A path ray that
 * hits a refractor from outside is shaded like any hit (lighting, weight *= reflectivity, one bounce) and continues along
 * the refracted direction; inside, the sphere is met at its far root; leaving it adds no colour and no weight but costs a
 * bounce; total internal reflection mirrors the ray; shadow rays are the reference's.  count must equal the scene's
 * sphere count when a frame is rendered; count = 0 turns the extension off.  Every ior[i] must lie in [0, 1e6): a call with
 * any other value -- negative, huge, infinite, not a number -- fails with TRT_ERR_ARGUMENT and leaves the extension off.
 *
 * THE DECLARED RULES (what a path ray remembers; tests/refraction_model.py is written from these, not from the kernel):
 *   - Only the sphere the ray most recently entered is remembered as the one it is `inside` of.
 *   - A ray that leaves a refractor nested in, or overlapping, another forgets the outer one: it then meets the outer one
 *     only at its near root, which lies behind it, so it passes that surface unbent.
 *   - The same holds for an eye that starts inside a refractor.
 *   - A ray inside a refractor that hits the ground or an opaque sphere reflects and stays inside.
 *   - eta is 1 / ior on entering and ior on leaving, relative to vacuum, whatever surrounds the sphere.
 *   - Total reflection, from inside or (ior < 1) from outside, keeps the side and the state.
 *   With the facing unit normal nn, d_n = (d . nn) nn, d_t = d - d_n and s2 = eta^2 |d_t|^2: s2 > 1 mirrors the ray about nn, which
 *   then starts 1e-6 BEFORE the surface like any reflected ray; otherwise the new direction is unit(eta d_t - sqrt(1 - s2) nn) from
 *   1e-6 PAST the surface, and the state becomes the sphere's index on entering, none on leaving.
 *
 * The extension is still UNPINNED TO THE REFERENCE, which has no refraction.  Frames are checked bit for bit against
 * oracle/trt_oracle.c's restatement of these very semantics, and that restatement is held, path ray by path ray, to an exact
 * (60-digit) model of the rules above (tests/test_refraction_model.py).  With the extension off (the default) a different
 * kernel instantiation runs and nothing of this is on the path. */
int trt_set_refraction(trt_context *ctx, const double *ior, int count);

/* EXTENSION, PARITY UNPINNED.  Specular highlights from Material.specularity, which the reference carries through every
 * Material and never reads: its author wrote the Blinn-Phong term into apply_lighting and left it commented out (TRT.c:913-916, :921,
 * :947-950, :955), and project_scene still forms the `view` vector the term needs (TRT.c:1029).  on = 1 switches the term on for the
 * frames this context renders, 0 (the default) off; anything else fails with TRT_ERR_ARGUMENT.
 *
 * THE DECLARED RULES (tests/specular_model.py is written from these, not from the kernel).  The lighting of a hit (TRT.c:894-962)
 * changes for every light i that reaches the surface point -- the same shadow test, unchanged --:
 *
 *     view  = -d                                      d: the path ray's direction as the round holds it, that is after
 *                                                     normalize_vector (TRT.c:1008 / :1055); TRT.c:1029
 *     half  = normalize_vector(light_direction + view)  light_direction first; the reference's normalisation, which leaves a vector
 *                                                     no longer than 1e-4 alone (TRT.c:444)
 *     c     = clamp(dot(normal, half), 0.0, 1.0)      the reference's clamp: a NaN passes through
 *     s     = powi(c, n)
 *     spec  = light.color * s                         directional light (TRT.c:916)
 *     spec  = light.color * (light_intensity * s)     point light (TRT.c:950): ONE product first, then the scale
 *     output_color += diffuse * material.color;  output_color += spec       in this order (TRT.c:920-921, :954-955)
 *
 * The term enters before the clamp of TRT.c:960 and is not multiplied by the material's colour.  n comes from the specularity e of
 * the hit material -- a sphere's, the even ground's or the odd ground's --: n = 0 if !(e >= 0), which covers negative values and NaN;
 * n = 65535 if e >= 65535; otherwise n = (int)e.  A FRACTIONAL EXPONENT IS TRUNCATED.  powi is binary exponentiation, right to left,
 * each product one rounded FP64 multiplication:
 *
 *     r = 1.0; b = c; while (n) { if (n & 1) r = r * b; n >>= 1; if (n) b = b * b; }
 *
 * so n = 0 gives 1.0, as pow(c, 0) does.  THIS IS THE ONE DEPARTURE from the commented-out lines, which call pow: pow is correctly
 * rounded neither in glibc nor in the device library, the two disagree in the last bits, and frames could not be held bit for bit.
 * powi is also the cheap form on the FP64 VALU: the demo's n = 100 is six squarings and two products.  Everything else -- shadow rays,
 * the diffuse term, weights, bounces and reflection, the sky, the nudge -- stays the reference's.
 *
 * The extension runs on the plain rounds (256-thread workgroups, never decoupled, with or without patches) and on the reference-order
 * kernel, as refraction does: a batch of cameras is served one launch per camera; a scene whose image outgrows LDS fails at render time
 * with TRT_ERR_CAPACITY; a render with this and the refraction extension both on fails with TRT_ERR_ARGUMENT -- the two do not combine
 * yet.  Every output kind (doubles, RGB8, the texts, kitty, sixel, the delta texts) works unchanged: they read the ordered mean.  The
 * trt_dist_* entries are out of scope: trt_dist_create and trt_dist_set_scene switch the extension off on every frame slot's context,
 * whatever TRT_SPECULAR says.  The switch is per context, like the refraction indices: trt_share_scene(dst, src) switches dst's OFF,
 * also when dst had it on from trt_set_specular or from the environment; call trt_set_specular(dst, 1) after sharing.
 * Environment: TRT_SPECULAR=0|1 sets the default of new contexts, until a trt_share_scene into them or a trt_set_specular.
 *
 * UNPINNED TO THE REFERENCE, whose live code has no such term.  Frames are checked bit for bit against tests/specular_restatement.c,
 * which with the switch off equals the oracle bit for bit, and whose every (hit, light) term is held to an exact model of the rules
 * above (tests/test_specular_model.py).  With the extension off other kernel instantiations run and nothing of this is on the path. */
int trt_set_specular(trt_context *ctx, int on);
int trt_get_specular(trt_context *ctx, int *on);
/* ... for the default context behind project_scene and the trt_render_frame_* entries (section 1), which their callers cannot reach:
 * holds for the default context that exists and for one a later call creates, until trt_shutdown.  Takes the default context's turn,
 * as trt_set_scene_policy does. */
int trt_set_default_specular(int on);

/* EXTENSION, PARITY UNPINNED.  Bilinear filtering of the sky.  get_skybox_color takes the nearest texel of a face, and directly under
 * that line its author wrote `//TODO->bicubic interpolation between the surrounding pixels in the texture` (TRT.c:786).  mode =
 * TRT_SKY_BILINEAR blends the four texels around the look-up for the frames this context renders, TRT_SKY_NEAREST (the default) is the
 * reference's path; anything else fails with TRT_ERR_ARGUMENT.  Four taps, clamped inside the face: no bicubic filter, no filtering
 * across the edges of the cube.
 *
 * THE DECLARED RULES (tests/sky_filter_model.py is written from these, not from the kernel).  Every step is one rounded binary64
 * operation, nothing contracted; clamp(a, lo, hi) is the reference's: a < lo ? lo : (a > hi ? hi : a).  dim is skybox.dim as a double.
 *
 *     f, u, v                                         the face and the coordinates of TRT.c:702-779, the clamp to +-0.5 included
 *     U = (u + 0.5) * dim;  V = (v + 0.5) * dim       TRT.c:782-783 before the truncation
 *     x = clamp(U - 0.5, 0.0, dim - 1.0)              texel centres lie at i + 0.5; the filter never leaves the face (clamp to edge)
 *     i0 = (int)x;  fx = x - (double)i0;  i1 = (i0 + 1 < dim) ? i0 + 1 : i0
 *     y, j0, fy, j1                                   likewise from V
 *     t00 = face[i0 + j0*dim]   t10 = face[i1 + j0*dim]   t01 = face[i0 + j1*dim]   t11 = face[i1 + j1*dim]
 *     per channel, the bytes converted to double:
 *     top = t00 + (t10 - t00) * fx;   bot = t01 + (t11 - t01) * fx;   c = (top + (bot - top) * fy) / 255.0
 *
 * f, u and v may be formed symbolically -- the products with the axis table's +-1 and 0 carried out on paper, as the nearest look-up
 * of the production kernel does: only the sign of a zero can differ, which u + 0.5 cannot see.  A direction with a component that is
 * not a number has no face in the reference and u, v that are not numbers: it gives face 0, all four taps texel 0 and fx = fy = 0, the
 * colour the nearest look-up defines for it; so does every direction whose u or v is not a number, which leaves the zero vector
 * (0 * inf) and vectors so short that dir * (1 / scale_by) overflows (a largest component below 2^-1024: the axis table's zeros then
 * meet inf).  The symbolic form holds these to the same answer by counting a u or v that is not FINITE before the clamp as not a number.  The lerp form, not a*(1-f) + b*f, on purpose: (a) four equal taps give exactly byte / 255.0, the reference's value;
 * (b) fx = fy = 0 gives exactly the texel (i0, j0) -- at a texel's centre the texel the nearest look-up returns --; (c) every channel
 * lies within [min, max] of its four taps over 255, so it never leaves [0, 1].
 *
 * The result replaces the colour of TRT.c:866; reflectivity and specularity of the miss stay 0.  Rays, shadow tests, weights and
 * bounces do not change: a frame's path-ray and shadow-ray counts are the oracle's.
 *
 * Like the specular extension it runs on the plain rounds (256-thread workgroups, never decoupled, with or without patches) and on the
 * reference-order kernel: a batch of cameras is served one launch per camera; a scene whose image outgrows LDS fails at render time
 * with TRT_ERR_CAPACITY; a render with the filter on and the refraction or the specular extension on fails with TRT_ERR_ARGUMENT -- they
 * do not combine yet.  Every output kind works unchanged: they read the ordered mean.  trt_dist_create and trt_dist_set_scene switch
 * it off on every frame slot's context; trt_share_scene(dst, src) switches dst's off.  Environment: TRT_SKY_FILTER=0|1 sets the
 * default of new contexts.
 *
 * UNPINNED TO THE REFERENCE, which has no filter.  Frames are checked bit for bit against tests/sky_filter_restatement.c, which with
 * the switch off equals the oracle bit for bit and whose every look-up is held to an exact model of the rules above
 * (tests/test_sky_filter_model.py).  With the filter off other kernel instantiations run and nothing of this is on the path. */
#define TRT_SKY_NEAREST 0
#define TRT_SKY_BILINEAR 1
int trt_set_sky_filter(trt_context *ctx, int mode);
int trt_get_sky_filter(trt_context *ctx, int *mode);
/* ... for the default context, as trt_set_default_specular is. */
int trt_set_default_sky_filter(int mode);

/* Resource usage of the render kernel trt_render_variant describes (hipFuncGetAttributes / occupancy query; max_blocks_per_cu
 * counts workgroups of trt_render_variant's size, and for 256-thread workgroups is the plain rounds' figure, which sizes them). */
int trt_kernel_info(trt_context *ctx, int *vgprs, int *sgprs, int *static_lds_bytes, int *max_blocks_per_cu,
                    int *compute_units);

const char *trt_last_error(void);
const char *trt_version(void);

/* ---- 3. one frame over the GPUs of a node (csrc/trt_dist.hip) --------------------------------- */

/* The reference renders a frame with one call, project_scene (TRT.c:966), from its single call site TRT.c:1339; every
 * pixel is independent.  Here one rank = one process (or thread) = one GPU; the ranks render interleaved tiles of
 * `tile_rows` rows each (tile t -> rank t mod world) and ONE gather per frame brings the rows to rank 0 over RCCL
 * (ncclSend / ncclRecv inside one group on the library's own stream; over xGMI every peer has its own link to the root).
 * Frames are pipelined over `frames_in_flight` renderer contexts.  RCCL is loaded at run time (librccl.so.1) and only for
 * world > 1.  (Test hook, include/trt_hip_diag.h: a process that asks for it before its first use of RCCL binds the library the
 * environment variable TRT_RCCL_LIB names instead -- the tests' stand-in, which lets several ranks share one GPU; every other
 * process ignores the variable.)
 * The host program carries the 128-byte id from rank 0 to the other ranks however it likes (MPI, a file, a socket,
 * torch.distributed): it is what ncclGetUniqueId produced. */
typedef struct trt_dist trt_dist;
#define TRT_DIST_ID_BYTES 128

int trt_dist_unique_id(void *id_out); /* rank 0 */
/* The library this process bound for the collectives ("" before the first use; "STAND-IN (TRT_RCCL_LIB): <path>" when the test
 * hook of trt_hip_diag.h took effect). */
const char *trt_dist_rccl_library(void);

/* Collective over the `world` ranks (same id, world, frame size, tile_rows everywhere).  scene: as for trt_set_scene (host
 * pointers inside; every rank holds the whole scene, ~1.5 MB with a 256^2 cubemap).  reserved_cus: compute units the
 * renderers leave to the collective's kernels (trt_reserve_cus; 0 = none).  id may be NULL when world == 1 (RCCL is then
 * not touched at all; with an id a one-rank communicator is created and the gather path runs with nobody to receive from). */
int trt_dist_create(int device, const Scene *scene, const void *id, int rank, int world, int width, int height, int tile_rows,
                    int frames_in_flight, int reserved_cus, trt_dist **out);
int trt_dist_set_scene(trt_dist *d, const Scene *scene);

/* Collective, asynchronous: this rank's rows of the frame seen from `camera` (TRT.c:1327-1339: a new camera per frame),
 * then the gather.  On rank 0 *d_frame is the DEVICE address of the assembled frame, height x width x 3 doubles in the
 * Screen layout of TRT.c:188-193 (NULL on the other ranks); it is complete after trt_dist_synchronize and is reused
 * `frames_in_flight` calls later. */
int trt_dist_render(trt_dist *d, const Camera *camera, int bounce_limit, int rays_per_pixel, void **d_frame);
/* If a collective fails on a rank (a HIP or RCCL error after the call has started to enqueue work), that rank is out of step
 * with its peers: the trt_dist is poisoned, every later render / synchronize call on it fails with TRT_ERR_NOT_INITIALISED,
 * and the host should destroy it on every rank. */
int trt_dist_synchronize(trt_dist *d);
/* The same frame as the 3 bytes per pixel the emitter makes of it ((int)(c*255), TRT.c:1157-1163): every rank
 * quantises its rows on the device and the gather moves bytes -- 8 times less over xGMI than doubles -- into an assembled
 * height x width x 3 byte frame on rank 0, bit-exact for buffered_draw_screen.  trt_dist_enable_rgb8 allocates the byte
 * buffers (once, on every rank, before the first trt_dist_render_rgb8); the two kinds of frame may be mixed. */
int trt_dist_enable_rgb8(trt_dist *d);
int trt_dist_render_rgb8(trt_dist *d, const Camera *camera, int bounce_limit, int rays_per_pixel, void **d_frame_rgb8);
int trt_dist_fetch_rgb8(trt_dist *d, const void *d_frame_rgb8, unsigned char *rgb);
/* synchronise, then copy an assembled frame into screen->pixels-like host memory (width*height Vectors) */
int trt_dist_fetch(trt_dist *d, const void *d_frame, Vector *pixels);
/* The root's assembly map, pure host arithmetic (no GPU): source_row[frame row] = row of the rank-major gather buffer in
 * which rank r's shard starts at row r * max_rows.  Returns max_rows, the height every shard is padded to. */
int trt_dist_source_rows(int width, int height, int tile_rows, int world, int *source_row);
int trt_dist_info(const trt_dist *d, int *rank, int *world, int *local_rows, int *max_rows, int *frames_in_flight);
/* How many ranks the communicator that was created has, as RCCL itself reports it (ncclCommCount; trt_dist_create fails unless
 * it equals `world`): the record that "RCCL saw N ranks".  0 when no communicator exists (world == 1 without an id). */
int trt_dist_comm_ranks(trt_dist *d);
/* Diagnostics, averaged over the frame slots' most recent frames (synchronises): this rank's render time (render kernel + ordered
 * mean) and the time its part of the gather took on the communicator's stream (send, or the receives and the assembly kernel on
 * the root); 0 where there was nothing to measure.  One number pair per rank makes a multi-GPU run diagnosable from one line. */
int trt_dist_frame_times(trt_dist *d, float *render_ms, float *gather_ms);
/* the renderer context of a slot (counters, kernel times, kernel selection); owned by d */
trt_context *trt_dist_context(trt_dist *d, int slot);
int trt_dist_destroy(trt_dist *d);
const char *trt_dist_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
