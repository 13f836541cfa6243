/*
 * sky_filter_restatement.c -- the frame producer with the sky filter, restated on the CPU in plain C.
 *
 * TEST INFRASTRUCTURE ONLY.  Written from the declared rules above trt_set_sky_filter in include/trt_hip.h and from the Scene layout of
 * include/trt.h; it shares no code with the kernels, with oracle/trt_oracle.c or with tests/sky_filter_model.py.  Build it as
 * tests/sky_filter_support.py does: gcc -O2 -ffp-contract=off -fno-fast-math.  Every floating-point operation is one rounded binary64
 * operation in the order the reference performs it ("TRT.c:N" = line N of TerminalRayTracer.c); the face and the coordinates of a
 * look-up are formed through the axis table, as TRT.c:702-779 form them.
 *
 * With `mode` = 0 a frame equals trt_oracle_project_scene's bit for bit (tests/test_sky_filter_model.py).  `mistake` plants one wrong
 * step in the filter (MISTAKE_*), for the tests that show that the model would notice.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "trt.h"

#define PI_ 3.14159265358979323846 /* TRT.c:43 */

enum
{
    MISTAKE_NONE = 0,
    MISTAKE_WEIGHTS_EXCHANGED = 1, /* fx where fy belongs and the other way round */
    MISTAKE_WEIGHTED_SUM = 2,      /* a*(1-f) + b*f in place of a + (b-a)*f */
    MISTAKE_NO_HALF_TEXEL = 3,     /* x = U, not U - 0.5 */
    MISTAKE_WRAP = 4,              /* i1 = (i0 + 1) % dim */
    MISTAKE_DIVIDE_FIRST = 5,      /* the taps divided by 255 before the blend */
    MISTAKE_TRANSPOSED = 6         /* face[j + i*dim] */
};

typedef struct
{
    unsigned long long path_rays;   /* rays of the bounce loop, TRT.c:1024 */
    unsigned long long shadow_rays; /* rays of the lighting, TRT.c:907, :937 */
} trt_sky_filter_stats;

/* One record per filtered look-up whose colour is used. */
enum
{
    LOOK_DIRECTION = 0, /* the direction as get_skybox_color receives it (3) */
    LOOK_FACE = 3,
    LOOK_I0 = 4,
    LOOK_J0 = 5,
    LOOK_I1 = 6,
    LOOK_J1 = 7,
    LOOK_FX = 8,
    LOOK_FY = 9,
    LOOK_TAPS = 10,   /* t00 t10 t01 t11, each r + 256 g + 65536 b (4) */
    LOOK_COLOUR = 14, /* (3) */
    LOOK_DOUBLES = 17
};

typedef struct
{
    double *looks; /* capacity * LOOK_DOUBLES doubles */
    size_t capacity;
    size_t count; /* look-ups met, also beyond capacity */
} trt_sky_filter_log;

typedef struct
{
    const Scene *scene;
    int mode, mistake;
    trt_sky_filter_stats *stats;
    trt_sky_filter_log *log;
} run;

static double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; } /* TRT.c:461 */

static void normalise(double *v) /* TRT.c:439-450 */
{
    double length = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (length > 0.0001)
    {
        v[0] /= length;
        v[1] /= length;
        v[2] /= length;
    }
}

static double clamp(double v, double lo, double hi) /* TRT.c:523-530: a NaN passes through */
{
    if (v < lo)
        return lo;
    if (v > hi)
        return hi;
    return v;
}

static void load(double *to, const void *from) { memcpy(to, from, 3 * sizeof(double)); }

/* TRT.c:638-672 */
static int meets_sphere(const double *o, const double *d, const Sphere *s, double *p)
{
    double oc[3] = {o[0] - s->center.x, o[1] - s->center.y, o[2] - s->center.z};
    double a = dot3(d, d);
    double b = 2.0 * dot3(oc, d);
    double c = dot3(oc, oc) - s->radius * s->radius;
    double discriminant = b * b - 4.0 * a * c;
    if (discriminant < 0.0)
        return 0;
    double t = (-b - sqrt(discriminant)) / (2.0 * a);
    if (!(t > 0.0))
        return 0;
    for (int k = 0; k < 3; k++)
        p[k] = o[k] + t * d[k];
    return 1;
}

/* TRT.c:677-695 */
static int meets_ground(const double *o, const double *d, const Plane *g, double *p)
{
    double n[3], at[3];
    load(n, &g->normal);
    load(at, &g->point);
    double denominator = dot3(d, n);
    if (!(fabs(denominator) > 0.00001))
        return 0;
    double to_plane[3] = {at[0] - o[0], at[1] - o[1], at[2] - o[2]};
    double t = dot3(to_plane, n) / denominator;
    if (!(t > 0.00001))
        return 0;
    for (int k = 0; k < 3; k++)
        p[k] = o[k] + t * d[k];
    return 1;
}

static const double AXES[6][3] = {{1.0, 0.0, 0.0}, {-1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, -1.0, 0.0}, {0.0, 0.0, 1.0}, {0.0, 0.0, -1.0}}; /* TRT.c:137-143 */

/* TRT.c:702-779: the face and the clamped coordinates a direction sees; face < 0 when no face wins (a direction that is not a number) */
static int face_and_coordinates(const double *direction, double *u_out, double *v_out)
{
    double dir[3] = {direction[0], direction[1], direction[2]};
    normalise(dir);
    int face = -1;
    double largest = -1.0;
    for (int f = 0; f < 6; f++)
    {
        double along = dot3(dir, AXES[f]);
        if (along > largest)
        {
            largest = along;
            face = f;
        }
    }
    if (face < 0)
    {
        *u_out = *v_out = NAN;
        return face;
    }
    double touching[3] = {dir[0] * AXES[face][0], dir[1] * AXES[face][1], dir[2] * AXES[face][2]};
    double by = 1.0 / (touching[0] + touching[1] + touching[2]);
    for (int k = 0; k < 3; k++)
        dir[k] = dir[k] * by;
    double along = dot3(dir, AXES[face]);
    double flat[3];
    for (int k = 0; k < 3; k++)
        flat[k] = (dir[k] - AXES[face][k] * along) * 0.5;
    double u = dot3(flat, AXES[(face + 2) % 6]);
    double v = dot3(flat, AXES[(face + 4) % 6]);
    if (face % 2 == 1)
        u *= -1.0;
    if (face < 2)
    {
        double t = u;
        u = v;
        v = -t;
    }
    else if (face < 4)
    {
        double t = u;
        u = -v;
        v = t;
    }
    else if (face == 4)
    {
        u *= -1.0;
        v *= -1.0;
    }
    *u_out = clamp(u, -0.5, 0.5);
    *v_out = clamp(v, -0.5, 0.5);
    return face;
}

/* TRT.c:780-789 and :866: the nearest texel, as a colour in [0, 1] */
static void nearest_colour(const Scene *scene, const double *direction, double *colour)
{
    double u, v;
    int face = face_and_coordinates(direction, &u, &v);
    if (face < 0) /* the reference reads outside its table; the project defines face 0 */
        face = 0;
    int dim = scene->skybox.dim;
    long at = 0, texels = (long)dim * dim;
    if (u == u && v == v)
    {
        int ui = (int)((u + 0.5) * dim);
        int vi = (int)((v + 0.5) * dim);
        at = (long)ui + (long)vi * dim;
    }
    if (at < 0) /* outside the face (u == 0.5 exactly): the reference reads past it; the project defines the nearest end */
        at = 0;
    if (at >= texels)
        at = texels - 1;
    Color texel = scene->skybox.colors[face][at];
    colour[0] = texel.r / 255.0;
    colour[1] = texel.g / 255.0;
    colour[2] = texel.b / 255.0;
}

/* one axis of the declared rules: the lower tap, the upper tap and the weight from U = (u + 0.5) * dim */
static void taps_of(double coordinate, int dim, int mistake, int *lower, int *upper, double *weight)
{
    double scaled = (coordinate + 0.5) * dim;
    double shifted = mistake == MISTAKE_NO_HALF_TEXEL ? scaled : scaled - 0.5;
    double x = clamp(shifted, 0.0, dim - 1.0);
    int i0 = (int)x;
    *lower = i0;
    *weight = x - (double)i0;
    if (mistake == MISTAKE_WRAP)
        *upper = (i0 + 1) % dim;
    else
        *upper = (i0 + 1 < dim) ? i0 + 1 : i0;
}

static double blend(double a, double b, double c, double d, double fx, double fy, int mistake)
{
    if (mistake == MISTAKE_DIVIDE_FIRST)
    {
        a = a / 255.0, b = b / 255.0, c = c / 255.0, d = d / 255.0;
        double top = a + (b - a) * fx;
        double bot = c + (d - c) * fx;
        return top + (bot - top) * fy;
    }
    if (mistake == MISTAKE_WEIGHTED_SUM)
    {
        double top = a * (1.0 - fx) + b * fx;
        double bot = c * (1.0 - fx) + d * fx;
        return (top * (1.0 - fy) + bot * fy) / 255.0;
    }
    double top = a + (b - a) * fx;
    double bot = c + (d - c) * fx;
    return (top + (bot - top) * fy) / 255.0;
}

static double packed(Color t) { return (double)(t.r + 256 * t.g + 65536 * t.b); }

/* the declared rules; `record`, if given, receives LOOK_DOUBLES doubles */
static void filtered_colour(const Scene *scene, const double *direction, int mistake, double *colour, double *record)
{
    double u, v, fx = 0.0, fy = 0.0;
    int face = face_and_coordinates(direction, &u, &v);
    int dim = scene->skybox.dim, i0 = 0, i1 = 0, j0 = 0, j1 = 0;
    if (face < 0 || !(u == u) || !(v == v)) /* not a number: face 0, four times texel 0, both weights 0 */
        face = 0;
    else
    {
        taps_of(u, dim, mistake, &i0, &i1, &fx);
        taps_of(v, dim, mistake, &j0, &j1, &fy);
    }
    const Color *texels = scene->skybox.colors[face];
    Color t00, t10, t01, t11;
    if (mistake == MISTAKE_TRANSPOSED)
        t00 = texels[j0 + (long)i0 * dim], t10 = texels[j0 + (long)i1 * dim], t01 = texels[j1 + (long)i0 * dim], t11 = texels[j1 + (long)i1 * dim];
    else
        t00 = texels[i0 + (long)j0 * dim], t10 = texels[i1 + (long)j0 * dim], t01 = texels[i0 + (long)j1 * dim], t11 = texels[i1 + (long)j1 * dim];
    double wx = mistake == MISTAKE_WEIGHTS_EXCHANGED ? fy : fx, wy = mistake == MISTAKE_WEIGHTS_EXCHANGED ? fx : fy;
    colour[0] = blend(t00.r, t10.r, t01.r, t11.r, wx, wy, mistake);
    colour[1] = blend(t00.g, t10.g, t01.g, t11.g, wx, wy, mistake);
    colour[2] = blend(t00.b, t10.b, t01.b, t11.b, wx, wy, mistake);
    if (record)
    {
        load(record + LOOK_DIRECTION, direction);
        record[LOOK_FACE] = face, record[LOOK_I0] = i0, record[LOOK_J0] = j0, record[LOOK_I1] = i1, record[LOOK_J1] = j1;
        record[LOOK_FX] = fx, record[LOOK_FY] = fy;
        record[LOOK_TAPS + 0] = packed(t00), record[LOOK_TAPS + 1] = packed(t10), record[LOOK_TAPS + 2] = packed(t01), record[LOOK_TAPS + 3] = packed(t11);
        load(record + LOOK_COLOUR, colour);
    }
}

static void sky_colour(const run *r, const double *direction, double *colour)
{
    if (!r->mode)
    {
        nearest_colour(r->scene, direction, colour);
        return;
    }
    trt_sky_filter_log *log = r->log;
    double *record = NULL;
    if (log)
    {
        if (log->count < log->capacity)
            record = log->looks + log->count * LOOK_DOUBLES;
        log->count++;
    }
    filtered_colour(r->scene, direction, r->mistake, colour, record);
}

typedef struct
{
    ObjectType what;
    double point[3];  /* pulled 1e-6 back towards the ray's origin; a miss: the origin */
    double normal[3]; /* normalised; a miss: the normalised direction */
    Material material;
} met;

/* TRT.c:793-889; a shadow ray (surface = 0) asks for neither normal nor material, and its sky colour is never read */
static met trace(const run *r, const double *o, const double *d, int surface)
{
    const Scene *scene = r->scene;
    met m;
    memset(&m, 0, sizeof m);
    m.what = NONE;
    double nearest = INFINITY, raw_normal[3] = {d[0], d[1], d[2]}, point[3] = {o[0], o[1], o[2]};
    for (int i = 0; i < scene->num_spheres; i++)
    {
        const Sphere *s = &scene->spheres[i];
        double p[3];
        if (!meets_sphere(o, d, s, p))
            continue;
        double back[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
        double distance2 = dot3(back, back);
        if (distance2 < nearest) /* the first of equals wins */
        {
            nearest = distance2;
            m.what = SPHERE;
            load(point, p);
            raw_normal[0] = p[0] - s->center.x, raw_normal[1] = p[1] - s->center.y, raw_normal[2] = p[2] - s->center.z;
            m.material = s->material;
        }
    }
    double p[3];
    if (meets_ground(o, d, &scene->ground, p))
    {
        double back[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
        double distance2 = dot3(back, back);
        if (distance2 < nearest)
        {
            nearest = distance2;
            m.what = GROUND;
            load(point, p);
            load(raw_normal, &scene->ground.normal);
            int odd = (int)(floor(p[0]) + floor(p[2])) & 1; /* TRT.c:850 */
            m.material = odd ? scene->ground.odd_material : scene->ground.even_material;
        }
    }
    if (m.what == NONE)
    {
        if (surface)
        {
            double c[3];
            sky_colour(r, d, c);
            m.material.color.x = c[0], m.material.color.y = c[1], m.material.color.z = c[2]; /* reflectivity and specularity 0, TRT.c:866 */
        }
    }
    else
    { /* TRT.c:868-875 */
        double back[3] = {o[0] - point[0], o[1] - point[1], o[2] - point[2]};
        normalise(back);
        for (int k = 0; k < 3; k++)
            point[k] = point[k] + back[k] * 0.000001;
    }
    load(m.point, point);
    normalise(raw_normal);
    load(m.normal, raw_normal);
    return m;
}

/* TRT.c:894-963 */
static void light(const run *r, const double *at, const double *normal, Material *material)
{
    const Scene *scene = r->scene;
    double out[3] = {0.0, 0.0, 0.0}, albedo[3];
    load(albedo, &material->color);
    for (int i = 0; i < scene->num_directional_lights; i++)
    {
        const DirectionalLight *l = &scene->directional_lights[i];
        double colour[3], light_direction[3] = {l->direction.x * -1.0, l->direction.y * -1.0, l->direction.z * -1.0};
        load(colour, &l->color);
        normalise(light_direction);
        r->stats->shadow_rays++;
        if (trace(r, at, light_direction, 0).what != NONE)
            continue;
        double diffuse = fmin(dot3(normal, light_direction), 1.0);
        for (int k = 0; k < 3; k++)
            out[k] = out[k] + (colour[k] * diffuse) * albedo[k];
    }
    for (int i = 0; i < scene->num_point_lights; i++)
    {
        const PointLight *l = &scene->point_lights[i];
        double colour[3], light_direction[3] = {l->position.x - at[0], l->position.y - at[1], l->position.z - at[2]};
        load(colour, &l->color);
        double light_distance2 = dot3(light_direction, light_direction);
        double light_intensity = clamp(l->intensity / light_distance2, 0.0, 1.0);
        normalise(light_direction);
        r->stats->shadow_rays++;
        met blocker = trace(r, at, light_direction, 0);
        double to_blocker[3] = {blocker.point[0] - at[0], blocker.point[1] - at[1], blocker.point[2] - at[2]};
        double blocker_distance2 = dot3(to_blocker, to_blocker);
        if (!(blocker.what == NONE || light_distance2 < blocker_distance2))
            continue;
        double diffuse = light_intensity * fmin(dot3(normal, light_direction), 1.0);
        for (int k = 0; k < 3; k++)
            out[k] = out[k] + (colour[k] * diffuse) * albedo[k];
    }
    material->color.x = clamp(out[0], 0.0, 1.0); /* TRT.c:960 */
    material->color.y = clamp(out[1], 0.0, 1.0);
    material->color.z = clamp(out[2], 0.0, 1.0);
}

static double triangle_wave(double t) /* TRT.c:225-228 */
{
    double m = fmod(t, 2 * PI_);
    return (m < PI_) ? (m / PI_) : (2 - (m / PI_));
}

/* TRT.c:966-1069 with BOUNCE_LIMIT and RAYS_PER_PIXEL as arguments; single-threaded, in the reference's pixel order */
void trt_sky_filter_project_scene(const Scene *scene, Screen *screen, int bounce_limit, int rays_per_pixel, int mode, int mistake,
                                  trt_sky_filter_stats *stats, trt_sky_filter_log *log)
{
    trt_sky_filter_stats local = {0, 0};
    run r = {scene, mode, mistake, stats ? stats : &local, mode ? log : NULL};
    r.stats->path_rays = r.stats->shadow_rays = 0;
    if (log)
        log->count = 0;
    const Camera *cam = &scene->camera;
    double bx[3], by[3], bz[3], eye[3];
    load(bx, &cam->frame.basis.x), load(by, &cam->frame.basis.y), load(bz, &cam->frame.basis.z), load(eye, &cam->frame.origin);
    for (int row = 0; row < screen->height; row++)
        for (int column = 0; column < screen->width; column++)
        {
            double mean[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < rays_per_pixel; k++)
            {
                double pixel_width = cam->screen_width / screen->width;
                double pixel_height = cam->screen_height / screen->height;
                double x = (((double)column / (double)screen->width) * cam->screen_width - cam->screen_width / 2.0);
                double y = -(((double)row / (double)screen->height) * cam->screen_height - cam->screen_height / 2.0);
                double z = -cam->screen_distance;
                x += triangle_wave(2 * PI_ * k / rays_per_pixel) / 2 * pixel_width;
                y += triangle_wave(PI_ * k / rays_per_pixel) / 2 * pixel_height;
                double d[3] = {0.0, 0.0, 0.0}, o[3];
                for (int c = 0; c < 3; c++)
                    d[c] = d[c] + bx[c] * x;
                for (int c = 0; c < 3; c++)
                    d[c] = d[c] + by[c] * y;
                for (int c = 0; c < 3; c++)
                    d[c] = d[c] + bz[c] * z;
                for (int c = 0; c < 3; c++)
                    d[c] = d[c] - eye[c]; /* sic, TRT.c:1005 */
                normalise(d);
                load(o, eye);
                double sample[3] = {0.0, 0.0, 0.0}, contribution = 1.0, contribution_total = 0.0;
                int bounces = 0, going = 1;
                while (going && bounces < bounce_limit && contribution > 0.00001)
                {
                    r.stats->path_rays++;
                    met m = trace(&r, o, d, 1);
                    if (m.what != NONE)
                        light(&r, m.point, m.normal, &m.material);
                    contribution_total += contribution;
                    double colour[3] = {m.material.color.x * contribution, m.material.color.y * contribution, m.material.color.z * contribution};
                    if (m.what != NONE)
                    {
                        contribution *= m.material.reflectivity;
                        bounces++;
                    }
                    else
                    {
                        contribution = 0.0;
                        going = 0;
                    }
                    for (int c = 0; c < 3; c++)
                        sample[c] = sample[c] + colour[c];
                    double along = dot3(d, m.normal); /* TRT.c:627-633 */
                    for (int c = 0; c < 3; c++)
                        d[c] = d[c] - 2.0 * along * m.normal[c];
                    normalise(d);
                    load(o, m.point);
                }
                double by_total = 1.0 / contribution_total;
                for (int c = 0; c < 3; c++)
                    mean[c] = mean[c] + sample[c] * by_total;
            }
            double by_rays = 1.0 / rays_per_pixel;
            Vector *px = &screen->pixels[(size_t)row * screen->width + column];
            px->x = mean[0] * by_rays, px->y = mean[1] * by_rays, px->z = mean[2] * by_rays;
        }
}

/* One ray as the probes report it: what it met and the material of TRT.c:866 / the hit (colour, reflectivity, specularity), unlit.
 * `record` (LOOK_DOUBLES doubles, or NULL) is filled when the ray ends on the sky with the filter on. */
int trt_sky_filter_shade_ray(const Scene *scene, const Ray *ray, int mode, int mistake, double *material, double *record)
{
    trt_sky_filter_stats st = {0, 0};
    trt_sky_filter_log one = {record, record ? 1 : 0, 0};
    run r = {scene, mode, mistake, &st, record && mode ? &one : NULL};
    double o[3], d[3];
    load(o, &ray->origin), load(d, &ray->direction);
    met m = trace(&r, o, d, 1);
    material[0] = m.material.color.x, material[1] = m.material.color.y, material[2] = m.material.color.z;
    material[3] = m.material.reflectivity, material[4] = m.material.specularity;
    return (int)m.what;
}

/* The filtered look-up of one direction alone (no scene geometry is read): colour (3) and the record. */
void trt_sky_filter_lookup(const Scene *scene, const double *direction, int mistake, double *colour, double *record)
{
    filtered_colour(scene, direction, mistake, colour, record);
}
