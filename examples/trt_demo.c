/* trt_demo.c -- the reference's frame loop (TRT.c:1235-1370) on top of libtrt_hip.so:
 * host C builds the demo scene and the orbiting camera, the MI355X produces the frame through
 * the drop-in project_scene(), and the ANSI emitter stays on the host.
 *
 *   trt_demo <skybox-directory> [frames=0 (until Ctrl-C)] [width=160] [height=48] [--no-draw] [--rgb8] [--ansi] [--half] [--kitty] [--sixel] [--256] [--delta] [--delta256]
 *            [--step=SECONDS] [--batch=N]
 *
 * --rgb8: the frame crosses PCIe as the 3 bytes per pixel the emitter makes of it (trt_render_frame_rgb8: the (int)(c*255) of
 * TRT.c:1157-1163 done on the device) instead of as 24-byte doubles; what reaches the terminal is the same.
 * --ansi: the frame crosses PCIe as the very text the terminal gets (trt_render_frame_ansi: the emitter's formatting done on the
 * device too), trt_ansi_bytes(width, height) bytes that one fwrite sends on; no trt_emitter on this route.
 * --half: the text route with two pixel rows per line of text (trt_render_frame_ansi_half): upper-half-block glyphs whose foreground is the
 * upper and whose background is the lower pixel, trt_ansi_half_bytes(width, height) bytes, one fwrite.  A pixel is one column by half a
 * line, which is square: the camera's screen_width = 5 * width / height is unchanged.  The terminal must be in a UTF-8 locale.
 * --kitty: true pixels for a terminal that speaks the kitty graphics protocol (trt_render_frame_kitty): base64 of the RGB bytes in APC escape
 * sequences, four bytes of text a pixel, trt_kitty_bytes(width, height) bytes, one fwrite per frame and nothing else on stdout; the image
 * replaces itself in place.  No terminal has yet shown this picture (csrc/trt_kitty.h).  It has no --delta form.
 * --sixel: true pixels for a terminal that takes DEC sixel (trt_render_frame_sixel): the 240 fixed colours of the xterm palette as colour
 * registers, the picture in bands of six rows; the length depends on the picture, so text has trt_sixel_capacity(width, height) bytes and
 * each frame is one fwrite of what the call reports, nothing else on stdout.  The terminal needs 256 colour registers (xterm:
 * numColorRegisters: 256).  No terminal has shown this picture (csrc/trt_sixel.h).  It has no --delta form.
 * --256: the text route for a terminal that has only the xterm 256-colour palette (trt_render_frame_ansi256; with --half
 * trt_render_frame_ansi256_half): "48;5;N" cells, N the entry of the palette's fixed part nearest to the pixel, no dithering;
 * trt_ansi256_bytes or trt_ansi256_half_bytes(width, height) bytes, one fwrite.  No terminal was at hand to look at this picture.  --256
 * sends whole texts and does not go with --delta: the palette's delta route has a flag of its own, --delta256.
 * --delta: the text route, but only what changed (trt_render_frame_ansi_delta): frame 0 arrives as the whole text, every later frame as the
 * records of the cells whose colour changed, each written with exactly the bytes the call reports.  Nothing else may be printed over
 * the picture, so the frames-per-second line goes to stderr once, at the end.
 * --half --delta: the same in half-block cells (trt_render_frame_ansi_delta_half): frame 0 arrives as --half's whole text, every later frame
 * as the records of the one-column cells either of whose two pixels changed.
 * --delta256: --delta in the xterm 256-colour palette (trt_render_frame_ansi256_delta; with --half trt_render_frame_ansi256_delta_half): frame 0
 * arrives as --256's whole text, every later frame as the records of the cells whose palette ENTRY changed -- fewer and shorter records than
 * --delta's, for the links where bytes per frame decide the frame rate.  Each frame is one fwrite of exactly the bytes the call reported.  It
 * goes with --half and --batch=N, and with none of --kitty, --sixel, --ansi and --rgb8.
 * --step=SECONDS: frame k is rendered at orbit time k * SECONDS instead of at the wall clock's (a replay: the same frames every run).
 * --batch=N, with --delta or --delta256 (with or without --half) and --step=: the replay rendered ahead, N cameras per call, through a context of
 * the program's own (trt_render_host_batch_ansi_delta, trt_render_host_batch_ansi_delta_half and their ansi256 forms): one render and three text kernels per N frames, two
 * transfers for their N texts, which are written frame by frame.  What reaches the terminal is byte for byte what --delta alone sends.
 * --specular: EXTENSION, parity unpinned (trt_set_default_specular; with --batch also trt_set_specular on the program's own context): the
 * lights' Blinn-Phong highlights from the specularity of 100.0 that the reference's scene gives every material and never reads.  Goes with
 * every other flag.
 * --sky-filter: EXTENSION, parity unpinned (trt_set_default_sky_filter; with --batch also trt_set_sky_filter): the sky blended from the
 * four texels around each look-up where the reference takes the nearest.  Goes with every other flag but --specular.
 *
 * The scene literals are the reference's (TRT.c:1256-1288). */
#include <signal.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "trt_hip.h"
#include "trt_host.h"

static volatile sig_atomic_t stop_requested = 0;
static void on_sigint(int sig)
{
    (void)sig;
    stop_requested = 1;
}

static double seconds_since(const struct timespec *start)
{
    struct timespec now;
    timespec_get(&now, TIME_UTC);
    return (double)(now.tv_sec - start->tv_sec) + (double)(now.tv_nsec - start->tv_nsec) / 1e9;
}

int main(int argc, char **argv)
{
    if (argc < 2)
    {
        fprintf(stderr, "usage: %s <skybox-directory> [frames] [width] [height] [--no-draw] [--rgb8] [--ansi] [--half] [--kitty] [--sixel] [--256] [--delta] [--delta256] [--step=SECONDS] [--batch=N] [--specular] [--sky-filter]\n", argv[0]);
        return 2;
    }
    const long frames = argc > 2 ? atol(argv[2]) : 0;
    const int width = argc > 3 ? atoi(argv[3]) : 160, height = argc > 4 ? atoi(argv[4]) : 48;
    int draw = 1, bytes_only = 0, text_only = 0, ansi = 0, delta = 0, delta256 = 0, half = 0, kitty = 0, sixel = 0, palette = 0, batch = 0, specular = 0, sky_filter = 0;
    double step = -1.0;
    for (int i = 5; i < argc; i++)
    {
        if (strcmp(argv[i], "--no-draw") == 0)
            draw = 0;
        else if (strcmp(argv[i], "--rgb8") == 0)
            bytes_only = 1;
        else if (strcmp(argv[i], "--ansi") == 0)
            text_only = ansi = 1;
        else if (strcmp(argv[i], "--half") == 0)
            text_only = half = 1;
        else if (strcmp(argv[i], "--kitty") == 0)
            text_only = kitty = 1;
        else if (strcmp(argv[i], "--sixel") == 0)
            text_only = sixel = 1;
        else if (strcmp(argv[i], "--256") == 0)
            text_only = palette = 1;
        else if (strcmp(argv[i], "--delta") == 0)
            text_only = delta = 1;
        else if (strcmp(argv[i], "--delta256") == 0)
            text_only = delta = delta256 = 1; /* a delta route: whatever holds of --delta below holds of it */
        else if (strncmp(argv[i], "--step=", 7) == 0)
            step = atof(argv[i] + 7);
        else if (strncmp(argv[i], "--batch=", 8) == 0)
            batch = atoi(argv[i] + 8);
        else if (strcmp(argv[i], "--specular") == 0)
            specular = 1; /* EXTENSION, parity unpinned: highlights from Material.specularity; goes with every other flag */
        else if (strcmp(argv[i], "--sky-filter") == 0)
            sky_filter = 1; /* EXTENSION, parity unpinned: bilinear filtering of the sky */
    }
    if (batch && (batch < 1 || batch > TRT_BATCH_MAX || !delta || step < 0.0))
    {
        fprintf(stderr, "--batch=N renders a replay ahead: 1 <= N <= %d, with --delta or --delta256 and --step=SECONDS\n", TRT_BATCH_MAX);
        return 2;
    }
    if (kitty && (delta || half || trt_kitty_bytes(width, height) == 0))
    {
        fprintf(stderr, "--kitty sends whole images of at most 99999 x 99999 pixels: it goes with neither --delta nor --half\n");
        return 2;
    }
    if (sixel && (delta || half || kitty || palette || trt_sixel_capacity(width, height) == 0))
    {
        fprintf(stderr, "--sixel sends whole images of at most 99999 x 99999 pixels: it goes with none of --delta, --half, --kitty and --256\n");
        return 2;
    }
    if (palette && (delta || kitty))
    {
        fprintf(stderr, "--256 sends whole texts in the xterm palette: it goes with --half, with neither --delta nor --kitty; the palette's delta route is --delta256\n");
        return 2;
    }
    if (delta256 && (ansi || bytes_only))
    {
        fprintf(stderr, "--delta256 sends delta texts in the xterm palette: it goes with --half and --batch=N, with none of --kitty, --sixel, --ansi and --rgb8\n");
        return 2;
    }
    if (specular && sky_filter)
    {
        fprintf(stderr, "--specular and --sky-filter do not combine yet\n");
        return 2;
    }
    if (sky_filter && trt_set_default_sky_filter(TRT_SKY_BILINEAR) != TRT_OK)
    {
        fprintf(stderr, "trt_set_default_sky_filter: %s\n", trt_last_error());
        return 1;
    }
    if (specular && trt_set_default_specular(1) != TRT_OK)
    {
        fprintf(stderr, "trt_set_default_specular: %s\n", trt_last_error());
        return 1;
    }

    Skybox sky;
    int rc = trt_load_skybox(&sky, argv[1]);
    if (rc != TRT_HOST_OK)
    {
        fprintf(stderr, "cannot load skybox from %s (error %d)\n", argv[1], rc);
        return 1;
    }

    Sphere spheres[6] = {
        {{1.0, 0.0, 0.0}, 0.5, {{1.0, 0.0, 0.0}, 1.0, 100.0}},  {{0.0, 1.0, 0.0}, 0.5, {{0.0, 1.0, 0.0}, 0.8, 100.0}},
        {{0.0, 0.0, 1.0}, 0.5, {{0.0, 0.0, 1.0}, 0.8, 100.0}},  {{-1.0, 0.0, 0.0}, 0.5, {{0.0, 1.0, 1.0}, 0.8, 100.0}},
        {{0.0, -1.0, 0.0}, 0.5, {{1.0, 0.0, 1.0}, 0.8, 100.0}}, {{0.0, 0.0, -1.0}, 0.5, {{1.0, 1.0, 0.0}, 0.8, 100.0}},
    };
    DirectionalLight sun[1] = {{{-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}}};
    PointLight lamp[1] = {{{0.0, 0.0, 0.0}, {1.0, 1.0, 1.0}, 10.0}};

    Scene scene;
    memset(&scene, 0, sizeof scene);
    scene.spheres = spheres;
    scene.num_spheres = 6;
    scene.ground.point.y = -2.0;
    scene.ground.normal.y = 1.0;
    scene.ground.even_material = (Material){{1.0, 1.0, 1.0}, 0.2, 100.0};
    scene.ground.odd_material = (Material){{1.0, 0.0, 0.0}, 0.2, 100.0};
    scene.directional_lights = sun;
    scene.num_directional_lights = 1;
    scene.point_lights = lamp;
    scene.num_point_lights = 1;
    scene.skybox = sky;
    trt_init_camera(&scene.camera, width, height);

    Screen screen = {(Vector *)malloc(sizeof(Vector) * (size_t)width * height), width, height};
    unsigned char *rgb = (unsigned char *)malloc((size_t)width * height * 3);
    /* the delta routes by kind: [--delta256][--half] */
    size_t (*const delta_capacity[2][2])(int, int) = {{trt_ansi_delta_capacity, trt_ansi_delta_half_capacity}, {trt_ansi256_delta_capacity, trt_ansi256_delta_half_capacity}};
    size_t (*const whole_bytes[2][2])(int, int) = {{trt_ansi_bytes, trt_ansi_half_bytes}, {trt_ansi256_bytes, trt_ansi256_half_bytes}};
    int (*const render_delta[2][2])(const Scene *, int, int, int, int, char *, size_t, size_t *) = {
        {trt_render_frame_ansi_delta, trt_render_frame_ansi_delta_half}, {trt_render_frame_ansi256_delta, trt_render_frame_ansi256_delta_half}};
    int (*const render_batch_delta[2][2])(trt_context *, const Camera *, int, const trt_rowset *, int, int, char *, size_t, size_t *) = {
        {trt_render_host_batch_ansi_delta, trt_render_host_batch_ansi_delta_half}, {trt_render_host_batch_ansi256_delta, trt_render_host_batch_ansi256_delta_half}};
    const char *const delta_name[2][2] = {{"ansi_delta", "ansi_delta_half"}, {"ansi256_delta", "ansi256_delta_half"}};
    const size_t text_room = delta  ? (size_t)(batch ? batch : 1) * delta_capacity[delta256][half](width, height)
                             : palette ? (half ? trt_ansi256_half_bytes(width, height) : trt_ansi256_bytes(width, height))
                             : half  ? trt_ansi_half_bytes(width, height)
                             : kitty ? trt_kitty_bytes(width, height)
                             : sixel ? trt_sixel_capacity(width, height)
                                    : trt_ansi_bytes(width, height);
    size_t text_bytes = text_room, written_bytes = 0;
    char *text = (char *)malloc(text_room ? text_room : 1);
    trt_emitter *emitter = NULL;
    if (!screen.pixels || !rgb || !text || (!text_only && trt_emitter_create(width, height, &emitter) != TRT_HOST_OK))
        return 1;

    /* --batch: a context of the program's own, the scene handed over once; the cameras of a batch and the lengths of their texts */
    trt_context *ctx = NULL;
    const trt_rowset whole = {width, height, height, 0, 1};
    Camera cameras[TRT_BATCH_MAX];
    size_t batch_bytes[TRT_BATCH_MAX];
    if (batch && (trt_create(0, &ctx) != TRT_OK || trt_set_scene(ctx, &scene) != TRT_OK || trt_set_specular(ctx, specular) != TRT_OK ||
                  trt_set_sky_filter(ctx, sky_filter) != TRT_OK))
    {
        fprintf(stderr, "trt_create / trt_set_scene / trt_set_specular / trt_set_sky_filter: %s\n", trt_last_error());
        return 1;
    }

    signal(SIGINT, on_sigint);
    struct timespec start;
    timespec_get(&start, TIME_UTC);
    double producer_seconds = 0.0, first_call_seconds = 0.0;
    long frame = 0;
    while (batch && !stop_requested && (frames == 0 || frame < frames))
    { /* the next `n` frames of the replay in one call, their texts back to back */
        const int n = frames == 0 || frames - frame > batch ? batch : (int)(frames - frame);
        for (int b = 0; b < n; b++)
        {
            trt_orbit_camera(&scene.camera, step * (double)(frame + b));
            cameras[b] = scene.camera;
        }
        const double before = seconds_since(&start);
        if (render_batch_delta[delta256][half](ctx, cameras, n, &whole, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text, text_room, batch_bytes) != TRT_OK)
        {
            fprintf(stderr, "trt_render_host_batch_%s: %s\n", delta_name[delta256][half], trt_last_error());
            return 1;
        }
        if (frame == 0) /* as below: initialisation is in the first call, which here is a whole batch */
            first_call_seconds = seconds_since(&start) - before;
        else
            producer_seconds += seconds_since(&start) - before;
        size_t at = 0;
        for (int b = 0; b < n; at += batch_bytes[b], b++)
            if (draw)
            {
                written_bytes += fwrite(text + at, 1, batch_bytes[b], stdout);
                fflush(stdout);
            }
        frame += n;
    }
    const long first_batch = batch && frame ? (frame < batch ? frame : batch) : 1; /* frames of the first call, which producer_seconds leaves out */
    for (; !batch && !stop_requested && (frames == 0 || frame < frames); frame++)
    {
        const double t = seconds_since(&start);
        trt_orbit_camera(&scene.camera, step >= 0.0 ? step * (double)frame : t);

        const double before = seconds_since(&start);
        if (delta)
        {
            if (render_delta[delta256][half](&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text, text_room, &text_bytes) != TRT_OK)
            {
                fprintf(stderr, "trt_render_frame_%s: %s\n", delta_name[delta256][half], trt_last_error());
                return 1;
            }
        }
        else if (palette)
        {
            if ((half ? trt_render_frame_ansi256_half : trt_render_frame_ansi256)(&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text) != TRT_OK)
            {
                fprintf(stderr, "trt_render_frame_ansi256%s: %s\n", half ? "_half" : "", trt_last_error());
                return 1;
            }
        }
        else if (half)
        {
            if (trt_render_frame_ansi_half(&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text) != TRT_OK)
            {
                fprintf(stderr, "trt_render_frame_ansi_half: %s\n", trt_last_error());
                return 1;
            }
        }
        else if (kitty)
        {
            if (trt_render_frame_kitty(&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text) != TRT_OK)
            {
                fprintf(stderr, "trt_render_frame_kitty: %s\n", trt_last_error());
                return 1;
            }
        }
        else if (sixel)
        {
            if (trt_render_frame_sixel(&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text, text_room, &text_bytes) != TRT_OK)
            {
                fprintf(stderr, "trt_render_frame_sixel: %s\n", trt_last_error());
                return 1;
            }
        }
        else if (text_only)
        {
            if (trt_render_frame_ansi(&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, text) != TRT_OK)
            {
                fprintf(stderr, "trt_render_frame_ansi: %s\n", trt_last_error());
                return 1;
            }
        }
        else if (!bytes_only)
            project_scene(&scene, &screen); /* the GPU frame producer, same call as TRT.c:1339 */
        else if (trt_render_frame_rgb8(&scene, width, height, TRT_REF_BOUNCE_LIMIT, TRT_REF_RAYS_PER_PIXEL, rgb) != TRT_OK)
        {
            fprintf(stderr, "trt_render_frame_rgb8: %s\n", trt_last_error());
            return 1;
        }
        if (frame == 0) /* device initialisation, cubemap upload and pinned staging happen in the first call */
            first_call_seconds = seconds_since(&start) - before;
        else
            producer_seconds += seconds_since(&start) - before;

        if (draw)
        {
            if (text_only)
                written_bytes += fwrite(text, 1, text_bytes, stdout); /* --ansi: sizeof(screenbuffer), NULs included, as TRT.c:1171; --half, --kitty, --256: the whole text; --delta, --sixel: what the call reported */
            else
            {
                if (bytes_only)
                    trt_emitter_patch_rgb8(emitter, rgb);
                else
                    trt_emitter_patch(emitter, &screen);
                trt_emitter_write(emitter, stdout);
            }
            if (delta || kitty || sixel)
                fflush(stdout); /* a delta text ends wherever its last record does: nothing of it may wait for the next frame; an image stands alone */
            else
            {
                fputs("\033[0;0H", stdout);
                printf("%.02f fps\n", 1.0 / (seconds_since(&start) - t));
                fputs("\033[0;0H", stdout);
            }
        }
    }
    if (delta)
        fprintf(stderr, "\033[%d;1H\n%.02f fps, %zu bytes of text for %ld frames (%zu each as whole texts)\n", half ? (height + 1) / 2 : height,
                (double)frame / seconds_since(&start), written_bytes, frame, whole_bytes[delta256][half](width, height));
    fprintf(stderr, "%ld frames %dx%d, frame producer %.3f ms/frame after a first call of %.1f ms (host-in/host-out%s, 10 bounces, 10 rays per pixel)\n",
            frame, width, height, frame > first_batch ? 1e3 * producer_seconds / (frame - first_batch) : 0.0, 1e3 * first_call_seconds,
            delta256 && half ? " as half-block 256-colour delta text" : delta256 ? " as 256-colour delta text" : delta && half ? " as half-block delta text" : delta ? " as delta text" : palette && half ? " as half-block 256-colour text" : palette ? " as 256-colour text" : half ? " as half-block text" : kitty ? " as a kitty image" : sixel ? " as a sixel image" : text_only ? " as text" : bytes_only ? " as RGB8" : "");

    trt_emitter_destroy(emitter);
    free(screen.pixels);
    free(rgb);
    free(text);
    trt_free_skybox(&sky);
    if (ctx)
        trt_destroy(ctx);
    trt_shutdown();
    return 0;
}
