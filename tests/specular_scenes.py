"""Scene families of the specular extension (tests/test_specular_model.py on the CPU, tests/test_specular_gpu.py on the device).

Every frame is 64x36 at 3 rays per pixel (6912 samples: whole waves, several queue chunks) and 4 bounces.  Scenes are built relative
to the camera -- eye + right * x + up * y + fwd * z, refraction_scenes.frame_of -- and draw nothing at random."""
import numpy as np

import refraction_scenes as RS
import support as T
from terminalraytracer_amd import scenes as S

W, H, SPP, BOUNCES = RS.W, RS.H, RS.SPP, 4

# the exponents' wall: both clamps of n, the truncation, every bit length of the loop
SPECULARITIES = (0.0, 0.5, 1.0, 1.999, 2.0, 3.0, 7.0, 100.0, 255.0, 65534.5, 65535.0, 1e300, np.inf, -1.0, np.nan)


def camera():
    return T.bench_camera(W, H, 2.5)


def primary_direction(cam, row, column):
    """the unit direction of the first ray of pixel (row, column) -- triangle_wave(0) == 0: it has no jitter -- in the operation order of
    TRT.c:987-1008 (numpy's float64 arithmetic, one rounding per operation)"""
    v = T.screen_point(cam, W, H, row, column) - cam[9:12]
    length = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return v / length


def demo():
    """the reference's six spheres, ground and lights; every specularity is the reference's 100.0"""
    return S.demo_scene(T.sky("synth"), camera())


def _sphere(centre, radius, k, specularity, reflectivity=0.5):
    colour = [0.2 + 0.2 * (k % 4), 0.2 + 0.2 * ((k // 2) % 4), 0.2 + 0.2 * ((k // 3) % 4)]
    return [*centre, radius, *colour, reflectivity, specularity]


def _ground(even, odd):
    g = S.demo_ground().copy()
    g[10], g[15] = even, odd
    return g


def exponents():
    """a wall of 5 x 3 spheres, 0.9 apart, 3.5 ahead, whose specularities run through SPECULARITIES, lit by the demo's two lights (the
    point light hangs between the eye and the wall); the two ground materials have 1 and 1000.  A wave's 64 samples cover about 21
    pixels of a row: two or three spheres and the ground between them, so lanes whose n is exhausted sit beside running ones."""
    cam = camera()
    eye, right, up, fwd = RS.frame_of(cam)
    rows = [_sphere(eye + right * (0.9 * (k % 5 - 2)) + up * (0.9 * (k // 5 - 1)) + fwd * 3.5, 0.4, k, e) for k, e in enumerate(SPECULARITIES)]
    d, p = S.demo_lights()
    return S.SceneData(np.array(rows), _ground(1.0, 1000.0), d, p, cam, T.sky("synth"))


# pixels whose first ray a light of the grazing family is laid along, and pixels whose first ray runs through a sphere's centre
GRAZING_ALONG = ((30, 8), (30, 24), (31, 40), (33, 56))
GRAZING_HEAD_ON = tuple((row, column) for row in (4, 8, 12, 16, 20, 24) for column in (5, 14, 23, 32, 41, 50, 59))


def grazing():
    """Where the term's two guards act.
    - Four directional lights that shine UP along the first ray of a ground pixel each (GRAZING_ALONG): light_direction is that ray's
      own direction, view its opposite, their sum no longer than 1e-4, and the reference's normalisation leaves `half` alone.  The
      ground does not shadow such a light: the shadow ray starts 1e-6 back along the ray and meets the plane below the 1e-5 of
      TRT.c:690.  At the ground hits around, half = light_direction - d points below the surface wherever the light is the steeper of
      the two: dot(normal, half) is negative and the clamp acts.
    - A point light AT THE EYE and 42 small spheres whose centres lie on the first rays of GRAZING_HEAD_ON: there the normal, the view
      and light_direction are one direction up to rounding, so dot(normal, half) is 1 give or take its last bit -- above 1 at about
      one such hit in six, where the clamp acts.
    The ground materials have specularity 0 (s = 1: the whole colour of the light) and 1 (s = c)."""
    cam = camera()
    eye = cam[9:12].copy()
    rows = []
    for k, (row, column) in enumerate(GRAZING_HEAD_ON):
        rows.append(_sphere(eye + primary_direction(cam, row, column) * (3.0 + 0.25 * (k % 3)), 0.2, k, (1.0, 2.0, 100.0)[k % 3]))
    d = np.array([[*(-primary_direction(cam, row, column)), 0.2, 0.15, 0.1] for row, column in GRAZING_ALONG])
    p = np.array([[*eye, 0.6, 0.7, 0.8, 4.0]])
    return S.SceneData(np.array(rows), _ground(0.0, 1.0), d, p, cam, T.sky("synth"))


def _lights_scene(n_dir, n_point):
    """the demo's spheres and ground under support.SWEEP_DIR_LIGHTS / SWEEP_POINT_LIGHTS: the first point light with an intensity at
    which light_intensity clamps to 1 everywhere, the second, 45 above the scene, one at which it never does"""
    p = T.SWEEP_POINT_LIGHTS.copy()
    p[0, 6] = 1e5
    point = p[1:2] if n_point == 1 else p[:n_point]
    return S.SceneData(S.demo_spheres(), S.demo_ground(), T.SWEEP_DIR_LIGHTS[:n_dir], point, camera(), T.sky("synth"))


def dense():
    """130 spheres: the patches instantiations run with tables in use"""
    return T.sweep_scene(130).with_camera(camera())


FAMILIES = {"demo": demo, "exponents": exponents, "grazing": grazing, "no lights": lambda: _lights_scene(0, 0),
            "one directional light": lambda: _lights_scene(1, 0), "one point light": lambda: _lights_scene(0, 1),
            "three and two lights": lambda: _lights_scene(3, 2), "dense": dense}


def aimed_rays(scene):
    """about 2 000 unit rays from the eye: a disc of 81 aims over each of the first twenty spheres -- its middle first, then out to 0.95
    of the radius, the limb included -- and a fan over the ground and the rest"""
    cam = scene.camera
    eye, right, up, fwd = RS.frame_of(cam)
    rays = []
    offsets = [(0.0, 0.0)] + [(a / 5.0, b / 5.0) for a in range(-5, 6) for b in range(-5, 6) if (a or b) and a * a + b * b <= 25]
    for sphere in scene.spheres[:20]:
        for a, b in offsets:
            v = sphere[:3] + 0.95 * sphere[3] * (a * right + b * up) - eye
            rays.append(np.concatenate([eye, v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])]))
    for i in range(2000 - len(rays)):
        v = fwd + right * (0.02 * (i % 41) - 0.4) - up * (0.15 + 0.01 * (i // 41))
        rays.append(np.concatenate([eye, v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])]))
    return np.array(rays)
