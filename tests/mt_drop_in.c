/* mt_drop_in.c -- test helper: project_scene() from four threads at once, EACH WITH A SCENE OF ITS OWN (the drop-in layer shares one
 * context and takes turns); compiled and run by tests/test_gpu_parity.py.
 *
 * The reference's project_scene is a pure function of *scene (TRT.c:966).  Here the default context thrashes between four scenes
 * -- 2, 40, 130 and 300 spheres, the last with a cubemap of its own -- so every call finds another scene's primitives, tables, skybox
 * and eye tables in place.  Each thread holds every frame it gets against the frame this program rendered for its scene before the
 * threads started.  The first two rounds go strictly in turn, so that every call is a change and the layer must come to treat its
 * scene as moving (trt_scene_is_moving() == 1: reported); the other rounds run freely and contend for the lock. */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "trt.h"
#include "trt_hip.h"
#include "trt_host.h"

enum { THREADS = 4, ROUNDS = 5, IN_TURN = 2, W = 96, H = 54 };
static const int kSpheres[THREADS] = {2, 40, 130, 300};

typedef struct
{
    Scene scene;
    Vector *expected; /* rendered before the threads start */
    int id, wrong_frames, saw_moving;
} Caller;

static Caller callers[THREADS];
static pthread_mutex_t turn_lock = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t turn_moved = PTHREAD_COND_INITIALIZER;
static int turn = 0; /* calls made so far in the rounds that go in turn */

static double unit(unsigned long long *state) /* splitmix64, as the SYNTH scenes use it */
{
    unsigned long long z = (*state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (double)((z ^ (z >> 31)) >> 11) * (1.0 / 9007199254740992.0);
}

static void make_scene(Caller *c, const Skybox *sky)
{
    static DirectionalLight sun = {{-1, -1, -1}, {1, 1, 1}};
    unsigned long long state = 1234 + (unsigned long long)c->id;
    const int n = kSpheres[c->id];
    Sphere *sp = malloc(sizeof(Sphere) * n);
    for (int i = 0; i < n; i++)
    {
        sp[i].center = (Point){8 * unit(&state) - 4, 4 * unit(&state) - 1.5, 8 * unit(&state) - 4.5};
        sp[i].radius = 0.1 + 0.4 * unit(&state);
        sp[i].material = (Material){{unit(&state), unit(&state), unit(&state)}, unit(&state), 100};
    }
    memset(&c->scene, 0, sizeof c->scene);
    c->scene.spheres = sp;
    c->scene.num_spheres = n;
    c->scene.directional_lights = &sun;
    c->scene.num_directional_lights = 1;
    c->scene.ground.point = (Point){0, -2, 0};
    c->scene.ground.normal = (Vector){0, 1, 0};
    c->scene.ground.even_material = (Material){{1, 1, 1}, 0.2, 100};
    c->scene.ground.odd_material = (Material){{0, 0, 0}, 0.2, 100};
    c->scene.skybox = *sky;
    trt_init_camera(&c->scene.camera, W, H);
    trt_orbit_camera(&c->scene.camera, 1.0 + 0.5 * c->id);
}

static void *work(void *arg)
{
    Caller *c = arg;
    Screen s = {malloc(sizeof(Vector) * W * H), W, H};
    for (int round = 0; round < ROUNDS; round++)
    {
        if (round < IN_TURN)
        {
            pthread_mutex_lock(&turn_lock);
            while (turn != round * THREADS + c->id)
                pthread_cond_wait(&turn_moved, &turn_lock);
            pthread_mutex_unlock(&turn_lock);
        }
        project_scene(&c->scene, &s);
        if (round < IN_TURN)
        {
            c->saw_moving |= trt_scene_is_moving(); /* nobody else calls before the turn is passed on */
            pthread_mutex_lock(&turn_lock);
            turn++;
            pthread_cond_broadcast(&turn_moved);
            pthread_mutex_unlock(&turn_lock);
        }
        c->wrong_frames += memcmp(s.pixels, c->expected, sizeof(Vector) * W * H) != 0;
    }
    free(s.pixels);
    return NULL;
}

int main(void)
{
    static Color shared_texels[6][16], own_texels[6][64];
    Skybox shared_sky, own_sky;
    for (int f = 0; f < 6; f++)
    {
        for (int i = 0; i < 16; i++)
            shared_texels[f][i] = (Color){(unsigned char)(40 * f), 100, (unsigned char)(10 * i)};
        for (int i = 0; i < 64; i++)
            own_texels[f][i] = (Color){(unsigned char)(3 * i), (unsigned char)(200 - 30 * f), 60};
        shared_sky.colors[f] = shared_texels[f];
        own_sky.colors[f] = own_texels[f];
    }
    shared_sky.dim = 4;
    own_sky.dim = 8;
    for (int k = 0; k < THREADS; k++)
    {
        callers[k].id = k;
        make_scene(&callers[k], k == THREADS - 1 ? &own_sky : &shared_sky);
        Screen s = {malloc(sizeof(Vector) * W * H), W, H};
        project_scene(&callers[k].scene, &s);
        callers[k].expected = s.pixels;
    }
    int distinct = 1; /* four scenes, four frames: the comparison below is not between copies of one frame */
    for (int k = 1; k < THREADS; k++)
        distinct &= memcmp(callers[0].expected, callers[k].expected, sizeof(Vector) * W * H) != 0;
    trt_shutdown(); /* the threads start on a fresh default context */
    pthread_t t[THREADS];
    for (int k = 0; k < THREADS; k++)
        pthread_create(&t[k], NULL, work, &callers[k]);
    for (int k = 0; k < THREADS; k++)
        pthread_join(t[k], NULL);
    int wrong = 0, moving = 0;
    for (int k = 0; k < THREADS; k++)
    {
        wrong += callers[k].wrong_frames;
        moving |= callers[k].saw_moving;
    }
    printf("4 threads x 5 project_scene calls, a scene each (%d, %d, %d, %d spheres): frames %s, the scenes' frames %s, scene %s\n", kSpheres[0],
           kSpheres[1], kSpheres[2], kSpheres[3], wrong ? "DIFFER from the frame rendered before the threads started" : "identical to it",
           distinct ? "distinct" : "THE SAME", moving ? "became moving" : "NEVER MOVING");
    trt_shutdown();
    return wrong || !distinct || !moving;
}
