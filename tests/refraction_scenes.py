"""Scene families of the refraction extension (tests/test_refraction_model.py on the CPU, tests/test_refraction_gpu.py on the device).

The spheres are placed relative to the camera -- eye + right * x + up * y + fwd * z -- so that the refractors fill the view and most
samples bend at least once.  Every frame is 64x36 at 3 rays per pixel and 12 bounces (6912 samples: whole waves, several queue chunks);
the reflectivities lie between 0.8 and 0.95, so that a path ends at the bounce limit or on the sky, not on its weight.  Each builder
returns (scene, indices of refraction) and draws nothing at random."""
import numpy as np

import support as T
from terminalraytracer_amd import scenes as S

W, H, SPP, BOUNCES = 64, 36, 3, 12
WALL_INDICES = (1.5, 1.33, 2.4, 1.0, 0.7)
REFLECTIVITIES = (0.8, 0.85, 0.9, 0.95)


def camera():
    return T.bench_camera(W, H, 2.5)


def frame_of(cam):
    """(eye, right, up, fwd): a primary direction is right * sx + up * sy - z * distance - eye (TRT.c:996-1005), and the stored orbit
    cameras keep the eye on the basis' z axis, so the middle of the screen lies along -z"""
    eye, z = cam[9:12].copy(), cam[6:9].copy()
    assert np.abs(np.cross(eye, z)).max() < 1e-12, "the eye of a stored camera lies on the basis' z axis"
    return eye, cam[0:3].copy(), cam[3:6].copy(), -z


def look_at(eye, target, w=W, h=H, reach=2.99):
    """a camera at `eye` whose middle ray runs at `target`: the screen's middle, -z * distance, must be eye + reach * unit(target - eye)"""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    f = target - eye
    v = eye + reach * (f / np.sqrt(f @ f))
    distance = np.sqrt(v @ v)
    z = -v / distance
    x = np.cross([0.0, 1.0, 0.0], z)
    x = x / np.sqrt(x @ x)
    y = np.cross(z, x)
    return np.concatenate([x, y, z, eye, [distance, 5 * float(w) / float(h), 5.0]])


def _sphere(centre, radius, k):
    """sphere number k of a family: a colour and a reflectivity that depend on k alone"""
    colour = [0.25 + 0.25 * (k % 4), 0.25 + 0.25 * ((k // 2) % 4), 0.25 + 0.25 * ((k // 3) % 4)]
    return [*centre, radius, *colour, REFLECTIVITIES[k % 4], 100.0]


def _scene(rows, cam):
    ground = S.demo_ground().copy()
    ground[9] = ground[14] = 0.85
    d, p = S.demo_lights()
    return S.SceneData(np.array(rows, dtype=np.float64), ground, d, p, cam, T.sky("synth"))


def lens_wall(indices=WALL_INDICES):
    """3x4 spheres of radius 0.55, one unit apart (neighbours overlap), four units ahead, their indices cycling through `indices`; each
    holds, by turns, a concentric refractor of half its radius, an off-centre opaque mirror, a refractor that overlaps it by half a
    radius.  The lowest row dips into the floor."""
    cam = camera()
    eye, right, up, fwd = frame_of(cam)
    rows, ior = [], []
    for k in range(12):
        centre = eye + right * (k % 4 - 1.5) + up * (k // 4 - 1.0) + fwd * 4.0
        rows.append(_sphere(centre, 0.55, k))
        ior.append(indices[k % len(indices)])
    for k in range(12):
        centre, radius = np.array(rows[k][:3]), rows[k][3]
        inner = indices[(k + 2) % len(indices)]
        if k % 3 == 0:
            rows.append(_sphere(centre, 0.5 * radius, 12 + k))
            ior.append(inner)
        elif k % 3 == 1:
            rows.append(_sphere(centre + 0.2 * right - 0.1 * up, 0.2, 12 + k))
            rows[-1][7] = 0.95
            ior.append(0.0)
        else:
            small = 0.6 * radius
            away = -fwd + 0.5 * up
            away = away / np.sqrt(away @ away)
            rows.append(_sphere(centre + away * (radius + small - 0.5 * radius), small, 12 + k))
            ior.append(inner)
    return _scene(rows, cam), np.array(ior)


def dolls():
    """concentric refractors three deep (radii 1.6, 1.0, 0.5, the innermost 0.1 off centre) around an opaque core; two opaque spheres beside them"""
    cam = camera()
    eye, right, up, fwd = frame_of(cam)
    centre = eye + fwd * 3.2
    rows = [_sphere(centre, 1.6, 0), _sphere(centre, 1.0, 1), _sphere(centre + 0.1 * right, 0.5, 2), _sphere(centre + 0.1 * right, 0.2, 3),
            _sphere(centre + 2.6 * right + 0.3 * up, 0.7, 4), _sphere(centre - 2.5 * right + 0.8 * up, 0.6, 5)]
    return _scene(rows, cam), np.array([1.5, 1.33, 2.4, 0.0, 0.0, 0.0])


def eye_inside():
    """the eye inside a refractor of radius 2, which it never meets from within; a refractor inside that one, an opaque sphere outside"""
    cam = camera()
    eye, right, up, fwd = frame_of(cam)
    rows = [_sphere(eye + fwd * 0.5, 2.0, 0), _sphere(eye + fwd * 1.5 - 0.3 * right, 0.5, 1), _sphere(eye + fwd * 4.0 + 1.0 * right, 0.8, 2)]
    return _scene(rows, cam), np.array([1.5, 1.33, 0.0])


def grazing(index):
    """the eye 0.02 above a refractor of radius 10; a small sphere ahead above its horizon, another inside it"""
    cam = camera()
    eye, right, up, fwd = frame_of(cam)
    rows = [_sphere(eye - up * 10.02, 10.0, 0), _sphere(eye + fwd * 3.0 + up * 0.5 - right * 0.8, 0.4, 1), _sphere(eye + fwd * 4.0 - up * 1.5 + right * 0.6, 0.5, 2)]
    return _scene(rows, cam), np.array([index, 0.0, 0.0])


def old_scene(w=96, h=54):
    """the 24-sphere scene of test_refraction_extension_matches_its_cpu_restatement (tests/test_gpu_parity.py), unchanged"""
    base = S.synth_scene(24, T.sky("synth"), T.bench_camera(w, h, 2.5), seed=3)
    sph = base.spheres.copy()
    sph[5, :3] = sph[4, :3]
    sph[5, 3] = sph[4, 3] * 0.5
    sph[7, :3] = sph[6, :3] + [sph[6, 3] + sph[7, 3], 0.0, 0.0]
    sph[9, 1] = -2.0 + sph[9, 3] * 0.8
    ior = np.where(np.arange(24) % 3 == 0, 1.5, 0.0)
    ior[1], ior[2], ior[4], ior[7] = 0.7, 1.0, 1.33, 2.4
    return base.with_spheres(sph), ior


def floor():
    """the sphere of the old scene that dips into the floor (number 9, a refractor of index 1.5), a radius of 0.13, seen from 0.4 away"""
    scene, ior = old_scene(W, H)
    sph = scene.spheres.copy()
    sph[:, 7] = np.resize(REFLECTIVITIES, len(sph))
    ground = scene.ground.copy()
    ground[9] = ground[14] = 0.85
    target = sph[9, :3]
    cam = look_at(target + np.array([0.28, 0.2, 0.2]), target)
    return S.SceneData(sph, ground, scene.dir_lights, scene.point_lights, cam, scene.sky), ior


def many():
    """300 spheres, every third a refractor: 16-bit list entries, the 256-thread kernel with a large LDS image"""
    scene = S.synth_scene(300, T.sky("synth"), camera(), seed=11)
    return scene, np.where(np.arange(300) % 3 == 0, 1.5, 0.0)


EDGE_INDICES = (np.nan, np.inf, -1.5, 1e-200, 1e200, 5e-324, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0))


def index_accepted(v):
    """trt_set_refraction takes 0 <= ior < 1e6 and refuses everything else (TRT_ERR_ARGUMENT)"""
    return bool(0.0 <= v < 1e6)


def index_edges():
    """the lens wall with indices that are not numbers, infinite, negative, tiny, huge, denormal, one and the doubles either side of one"""
    return lens_wall(EDGE_INDICES)


def index_edges_accepted():
    """... with those of them the library accepts: tiny (eta^2 overflows), denormal (eta is infinite), one and its neighbours"""
    return lens_wall(tuple(v for v in EDGE_INDICES if index_accepted(v)))


# name: builder.  The device renders every family at (W, H, BOUNCES, SPP); the stored camera of 96x54 is that of 64x36 (16:9 both)
FAMILIES = {"lens wall": lens_wall, "dolls": dolls, "eye inside": eye_inside, "grazing 1.5": lambda: grazing(1.5), "grazing 0.7": lambda: grazing(0.7),
            "floor": floor, "old scene": old_scene}
GPU_ONLY = {"many": many, "index edges": index_edges_accepted}
# (width, height, bounce limit, rays per pixel) of the frame the exact model judges: the old scene keeps its old frame
MODEL_SHOT = {name: (96, 54, 10, 4) if name == "old scene" else (W, H, BOUNCES, SPP) for name in FAMILIES}
