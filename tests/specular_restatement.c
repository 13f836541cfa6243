/*
 * specular_restatement.c -- the frame producer with the specular extension, restated on the CPU in plain C.
 *
 * TEST INFRASTRUCTURE ONLY.  Written from the declared rules above trt_set_specular in include/trt_hip.h and from the Scene layout of
 * include/trt.h; it shares no code with the kernels, with oracle/trt_oracle.c or with tests/specular_model.py.  Build it as
 * tests/specular_support.py does: gcc -O2 -ffp-contract=off -fno-fast-math.  Every floating-point operation is one rounded binary64
 * operation in the order the reference performs it ("TRT.c:N" = line N of TerminalRayTracer.c); the lines of the specular term are the
 * ones the reference keeps commented out (TRT.c:913-916, :921, :947-950, :955), with powi where they call pow.
 *
 * With `on` = 0 a frame equals trt_oracle_project_scene's bit for bit (tests/test_specular_model.py).
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "trt.h"

#define PI_ 3.14159265358979323846 /* TRT.c:43 */

typedef struct
{
    unsigned long long path_rays;   /* rays of the bounce loop, TRT.c:1024 */
    unsigned long long shadow_rays; /* rays of the lighting, TRT.c:907, :937 */
} trt_specular_stats;

/* One record per shaded hit and light that reaches it: the doubles that enter the term and the spec that leaves it. */
enum
{
    TERM_D = 0,          /* the path ray's direction (3) */
    TERM_NORMAL = 3,     /* the unit normal (3) */
    TERM_LIGHT_DIR = 6,  /* light_direction, normalised (3) */
    TERM_INTENSITY = 9,  /* light_intensity (point lights; 1.0 and unused for a directional light) */
    TERM_COLOUR = 10,    /* the light's colour (3) */
    TERM_E = 13,         /* the hit material's specularity */
    TERM_POINT = 14,     /* 1.0: a point light, 0.0: a directional light */
    TERM_MATERIAL = 15,  /* the hit material's colour (3): not part of the term -- a planted mistake multiplies by it */
    TERM_SPEC = 18,      /* spec (3) */
    TERM_DOUBLES = 21
};

typedef struct
{
    double *terms; /* capacity * TERM_DOUBLES doubles */
    size_t capacity;
    size_t count; /* terms met, also beyond capacity */
} trt_specular_log;

typedef struct
{
    const Scene *scene;
    int on;
    trt_specular_stats *stats;
    trt_specular_log *log;
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

/* TRT.c:700-789: the texel a direction sees, as a colour in [0, 1] */
static void sky_colour(const Scene *scene, const double *direction, double *colour)
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
    if (face < 0) /* a direction that is not a number: the reference reads outside its table; the project defines face 0 */
        face = 0;
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
    u = clamp(u, -0.5, 0.5);
    v = clamp(v, -0.5, 0.5);
    int dim = scene->skybox.dim;
    int ui = (int)((u + 0.5) * dim);
    int vi = (int)((v + 0.5) * dim);
    long at = (long)ui + (long)vi * dim, texels = (long)dim * dim;
    if (at < 0) /* outside the face (u == 0.5 exactly): the reference reads past it; the project defines the nearest end */
        at = 0;
    if (at >= texels)
        at = texels - 1;
    Color texel = scene->skybox.colors[face][at];
    colour[0] = texel.r / 255.0;
    colour[1] = texel.g / 255.0;
    colour[2] = texel.b / 255.0;
}

typedef struct
{
    ObjectType what;
    double point[3];  /* pulled 1e-6 back towards the ray's origin; a miss: the origin */
    double normal[3]; /* normalised; a miss: the normalised direction */
    Material material;
} met;

/* TRT.c:793-889; a shadow ray (surface = 0) asks for neither normal nor material, and its sky colour is never read */
static met trace(const Scene *scene, const double *o, const double *d, int surface)
{
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
            sky_colour(scene, d, c);
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

/* the declared rules: n from the specularity, then c^n right to left */
static int exponent_of(double e)
{
    if (!(e >= 0.0))
        return 0;
    if (e >= 65535.0)
        return 65535;
    return (int)e;
}

static double powi(double c, int n)
{
    double r = 1.0, b = c;
    while (n)
    {
        if (n & 1)
            r = r * b;
        n >>= 1;
        if (n)
            b = b * b;
    }
    return r;
}

/* spec of one light (TRT.c:914-916 / :948-950), logged on request */
static void specular_term(const run *r, const double *d, const double *normal, const double *light_direction, double light_intensity, int point_light,
                          const double *light_colour, const Material *material, double *spec)
{
    double view[3] = {d[0] * -1.0, d[1] * -1.0, d[2] * -1.0}; /* TRT.c:1029 */
    double half[3] = {light_direction[0] + view[0], light_direction[1] + view[1], light_direction[2] + view[2]};
    normalise(half);
    double s = powi(clamp(dot3(normal, half), 0.0, 1.0), exponent_of(material->specularity));
    double by = point_light ? light_intensity * s : s;
    for (int k = 0; k < 3; k++)
        spec[k] = light_colour[k] * by;
    trt_specular_log *log = r->log;
    if (log)
    {
        if (log->count < log->capacity)
        {
            double *t = log->terms + log->count * TERM_DOUBLES;
            load(t + TERM_D, d), load(t + TERM_NORMAL, normal), load(t + TERM_LIGHT_DIR, light_direction), load(t + TERM_COLOUR, light_colour);
            t[TERM_INTENSITY] = point_light ? light_intensity : 1.0;
            t[TERM_E] = material->specularity;
            t[TERM_POINT] = point_light ? 1.0 : 0.0;
            load(t + TERM_MATERIAL, &material->color);
            load(t + TERM_SPEC, spec);
        }
        log->count++;
    }
}

/* TRT.c:894-963; d: the direction of the ray that met the point */
static void light(const run *r, const double *at, const double *d, const double *normal, Material *material)
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
        if (trace(scene, at, light_direction, 0).what != NONE)
            continue;
        double diffuse = fmin(dot3(normal, light_direction), 1.0);
        double spec[3] = {0.0, 0.0, 0.0};
        if (r->on)
            specular_term(r, d, normal, light_direction, 1.0, 0, colour, material, spec);
        for (int k = 0; k < 3; k++)
        {
            out[k] = out[k] + (colour[k] * diffuse) * albedo[k];
            if (r->on)
                out[k] = out[k] + spec[k];
        }
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
        met blocker = trace(scene, at, light_direction, 0);
        double to_blocker[3] = {blocker.point[0] - at[0], blocker.point[1] - at[1], blocker.point[2] - at[2]};
        double blocker_distance2 = dot3(to_blocker, to_blocker);
        if (!(blocker.what == NONE || light_distance2 < blocker_distance2))
            continue;
        double diffuse = light_intensity * fmin(dot3(normal, light_direction), 1.0);
        double spec[3] = {0.0, 0.0, 0.0};
        if (r->on)
            specular_term(r, d, normal, light_direction, light_intensity, 1, colour, material, spec);
        for (int k = 0; k < 3; k++)
        {
            out[k] = out[k] + (colour[k] * diffuse) * albedo[k];
            if (r->on)
                out[k] = out[k] + spec[k];
        }
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
void trt_specular_project_scene(const Scene *scene, Screen *screen, int bounce_limit, int rays_per_pixel, int on, trt_specular_stats *stats,
                                trt_specular_log *log)
{
    trt_specular_stats local = {0, 0};
    run r = {scene, on, stats ? stats : &local, on ? log : NULL};
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
                    met m = trace(scene, o, d, 1);
                    if (m.what != NONE)
                        light(&r, m.point, d, m.normal, &m.material);
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

/* One ray as the probes shade it: what it met, and the clamped colour of the point with the switch as given (0, 0, 0 on a miss).  The
 * view vector is minus the direction as it is given. */
int trt_specular_shade_ray(const Scene *scene, const Ray *ray, int on, double *lit)
{
    trt_specular_stats st = {0, 0};
    run r = {scene, on, &st, NULL};
    double o[3], d[3];
    load(o, &ray->origin), load(d, &ray->direction);
    met m = trace(scene, o, d, 1);
    lit[0] = lit[1] = lit[2] = 0.0;
    if (m.what != NONE)
    {
        light(&r, m.point, d, m.normal, &m.material);
        lit[0] = m.material.color.x, lit[1] = m.material.color.y, lit[2] = m.material.color.z;
    }
    return (int)m.what;
}
