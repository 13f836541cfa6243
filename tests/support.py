"""Shared test plumbing: the oracle binding (checker only), golden loaders, hashes, and the builders of the adversarial scenes
(nothing here needs a device)."""
import ctypes as C
import functools
import json
import os
import subprocess
import zlib

import numpy as np

from terminalraytracer_amd import hip
from terminalraytracer_amd import layout as L
from terminalraytracer_amd import scenes as S

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FACES = ["+X", "-X", "+Y", "-Y", "+Z", "-Z"]


# TRT_TEST_SANITIZE=1 (set by tests/test_sanitized.py for a child run): the host builds of the table headers (filter / light-table /
# ray-table checkers) are compiled with the address and undefined-behaviour sanitizers, under another name
SANITIZE = os.environ.get("TRT_TEST_SANITIZE") == "1"
CHECKER_FLAGS = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if SANITIZE else []


def checker_so(name):
    build = os.path.join(ROOT, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    return os.path.join(build, name + ("_san" if SANITIZE else "") + ".so")


@functools.lru_cache(maxsize=None)
def lightgrid_checker():
    """tests/lightgrid_check.c with the table headers it includes, compiled for the host: the one build recipe of its users"""
    so = checker_so("liblightgridcheck")
    src = os.path.join(ROOT, "tests", "lightgrid_check.c")
    inc = os.path.join(ROOT, "terminalraytracer_amd", "csrc")
    newest = max(os.path.getmtime(p) for p in [src] + [os.path.join(inc, h) for h in ("trt_raygrid.h", "trt_lightgrid.h", "trt_filter.h")])
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + CHECKER_FLAGS + ["-I" + inc, "-o", so, src, "-lm"])
    return C.CDLL(so)


class OracleStats(C.Structure):
    _fields_ = [("path_rays", C.c_ulonglong), ("shadow_rays", C.c_ulonglong), ("sky_lookups", C.c_ulonglong),
                ("samples", C.c_ulonglong)]


@functools.lru_cache(maxsize=None)
def oracle():
    """oracle/libtrt_oracle.so -- the CPU restatement.  Checker only; never on a product path."""
    path = os.environ.get("TRT_ORACLE_LIB") or os.path.join(ROOT, "oracle", "libtrt_oracle.so") # the variable: a sanitized build (test_oracle_golden.py)
    if not os.path.exists(path):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"])
    lib = C.CDLL(path)
    lib.trt_oracle_project_scene.argtypes = [C.POINTER(L.Scene), C.POINTER(L.Screen), C.c_int, C.c_int, C.c_int,
                                             C.POINTER(OracleStats)]
    lib.trt_oracle_project_scene.restype = None
    lib.trt_oracle_render_rows.argtypes = [C.POINTER(L.Scene), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.POINTER(OracleStats)]
    lib.trt_oracle_render_rows.restype = None
    lib.trt_oracle_trace_ray.argtypes = [C.POINTER(L.Scene), C.POINTER(L.Ray), C.POINTER(L.Vector), C.POINTER(L.Vector),
                                         C.POINTER(L.Material)]
    lib.trt_oracle_trace_ray.restype = C.c_int
    lib.trt_oracle_skybox_lookup.argtypes = [C.POINTER(L.Scene), C.POINTER(L.Vector), C.POINTER(C.c_int),
                                             C.POINTER(C.c_long)]
    lib.trt_oracle_skybox_lookup.restype = C.c_int
    lib.trt_oracle_apply_lighting.argtypes = [C.POINTER(L.Scene), C.POINTER(L.Vector), C.POINTER(L.Vector),
                                              C.POINTER(L.Material), C.POINTER(OracleStats)]
    lib.trt_oracle_apply_lighting.restype = None
    lib.trt_oracle_triangle_wave.argtypes = [C.c_double]
    lib.trt_oracle_triangle_wave.restype = C.c_double
    lib.trt_oracle_rgb8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    lib.trt_oracle_rgb8.restype = None
    lib.trt_oracle_fnv1a64.argtypes = [C.c_void_p, C.c_size_t]
    lib.trt_oracle_fnv1a64.restype = C.c_ulonglong
    lib.trt_oracle_div_sqrt.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.trt_oracle_div_sqrt.restype = None
    lib.trt_oracle_project_scene_refractive.argtypes = [C.POINTER(L.Scene), C.c_void_p, C.POINTER(L.Screen), C.c_int, C.c_int, C.c_int,
                                                        C.POINTER(OracleStats)]
    lib.trt_oracle_project_scene_refractive.restype = None
    return lib


def fnv(buf):
    a = np.ascontiguousarray(buf)
    return f"{oracle().trt_oracle_fnv1a64(a.ctypes.data, a.nbytes):016x}"


def oracle_render(scene_data, width, height, bounce_limit, rays_per_pixel, threads=None, rows=None):
    """(pixels[H,W,3] float64, stats) from the CPU restatement."""
    threads = threads or min(8, os.cpu_count() or 1)
    scene = scene_data.as_scene()
    st = OracleStats()
    if rows is None:
        screen, px = S.new_screen(width, height)
        oracle().trt_oracle_project_scene(C.byref(scene), C.byref(screen), bounce_limit, rays_per_pixel, threads, C.byref(st))
        return px, st
    r0, r1 = rows
    px = np.zeros((r1 - r0, width, 3), dtype=np.float64)
    oracle().trt_oracle_render_rows(C.byref(scene), px.ctypes.data, width, height, r0, r1, bounce_limit, rays_per_pixel,
                                    threads, C.byref(st))
    return px, st


def oracle_render_refractive(scene_data, ior, width, height, bounce_limit, rays_per_pixel, threads=None):
    """EXTENSION, parity unpinned: the oracle's restatement of the refraction variant (not the reference, which has none)."""
    threads = threads or min(8, os.cpu_count() or 1)
    scene = scene_data.as_scene()
    ior = np.ascontiguousarray(ior, dtype=np.float64)
    assert ior.size == scene_data.num_spheres
    st = OracleStats()
    screen, px = S.new_screen(width, height)
    oracle().trt_oracle_project_scene_refractive(C.byref(scene), ior.ctypes.data, C.byref(screen), bounce_limit, rays_per_pixel, threads, C.byref(st))
    return px, st


class OracleRayLog(C.Structure):
    _fields_ = [("rays", C.c_void_p), ("kinds", C.c_void_p), ("capacity", C.c_size_t), ("count", C.c_size_t)]


def oracle_path_rays_refractive(scene_data, ior, width, height, bounce_limit, rays_per_pixel):
    """(pixels, stats, path rays float64[n, 6]) of one single-threaded frame of the refraction restatement: every path ray it traces, in
    trace order (trt_oracle_set_ray_log; the shadow rays between them are dropped)"""
    cap = width * height * rays_per_pixel * bounce_limit * (1 + len(scene_data.dir_lights) + len(scene_data.point_lights)) + 1
    rays, kinds = np.zeros((cap, 6)), np.zeros(cap, dtype=np.uint8)
    log = OracleRayLog(rays.ctypes.data, kinds.ctypes.data, cap, 0)
    lib = oracle()
    lib.trt_oracle_set_ray_log.argtypes = [C.POINTER(OracleRayLog)]
    lib.trt_oracle_set_ray_log(C.byref(log))
    try:
        px, st = oracle_render_refractive(scene_data, ior, width, height, bounce_limit, rays_per_pixel, threads=1)
    finally:
        lib.trt_oracle_set_ray_log(None)
    assert log.count < cap
    return px, st, rays[: log.count][kinds[: log.count] == 0].copy()


ENDED_ON_SKY, ENDED_BY_LIMIT, ENDED_BY_WEIGHT = 0, 1, 2


def oracle_hit_sequences(scene_data, width, height, bounce_limit, rays_per_pixel, cameras=None):
    """What every sample of a small frame does, from one single-threaded oracle frame under the ray log: per work unit, in unit order
    (unit = pixel * rays_per_pixel + k; `cameras`: a batch, frame-major), the number of path rays, the number of hits (a path ray that
    shadow rays follow: the scene has a light) and how the sample ended (ENDED_*: the last ray met the sky; the last hit was the bounce
    limit's; the weight fell to 1e-5 or below).  Returns {"paths", "hits", "ending": int arrays, "frames": [pixels], "counts": (path
    rays, shadow rays) of all frames, "rays": per unit the float64[paths, 6] path rays}."""
    lights = len(scene_data.dir_lights) + len(scene_data.point_lights)
    assert lights >= 1 and bounce_limit >= 1
    samples = width * height * rays_per_pixel
    cap = samples * bounce_limit * (1 + lights) + 1
    lib = oracle()
    lib.trt_oracle_set_ray_log.argtypes = [C.POINTER(OracleRayLog)]
    paths, hits, ending, rays_of, frames, counts = [], [], [], [], [], [0, 0]
    for cam in ([scene_data.camera] if cameras is None else cameras):
        scene = scene_data.with_camera(cam)
        rays, kinds = np.zeros((cap, 6)), np.zeros(cap, dtype=np.uint8)
        log = OracleRayLog(rays.ctypes.data, kinds.ctypes.data, cap, 0)
        lib.trt_oracle_set_ray_log(C.byref(log))
        try:
            px, st = oracle_render(scene, width, height, bounce_limit, rays_per_pixel, threads=1)
        finally:
            lib.trt_oracle_set_ray_log(None)
        assert log.count < cap, "the ray log overflowed"
        rays, kinds = rays[: log.count], kinds[: log.count]
        path_at = np.nonzero(kinds == 0)[0]
        assert path_at.size == st.path_rays and log.count - path_at.size == st.shadow_rays
        is_hit = np.append(path_at[1:], log.count) - path_at > 1  # shadow rays follow
        # a sample's first path ray starts at the eye, bit for bit; no reflected ray does (it starts 1e-6 off a surface)
        first = np.nonzero((bits(rays[path_at, :3]) == bits(scene.camera[9:12])[None, :]).all(axis=1))[0]
        assert first.size == samples == st.samples, (first.size, samples, st.samples)
        assert first[0] == 0
        for a, b in zip(first, np.append(first[1:], path_at.size)):
            p, h = int(b - a), int(is_hit[a:b].sum())
            assert is_hit[a:a + h].all() and h in (p, p - 1) and 1 <= p <= bounce_limit  # hits, then at most one ray into the sky
            paths.append(p), hits.append(h), rays_of.append(rays[path_at[a:b]].copy())
            ending.append(ENDED_ON_SKY if h < p else ENDED_BY_LIMIT if h == bounce_limit else ENDED_BY_WEIGHT)
        px.setflags(write=False)
        frames.append(px)
        counts[0] += int(st.path_rays)
        counts[1] += int(st.shadow_rays)
    return {"paths": np.array(paths), "hits": np.array(hits), "ending": np.array(ending), "frames": frames, "counts": tuple(counts), "rays": rays_of}


def oracle_rgb8(pixels):
    px = np.ascontiguousarray(pixels, dtype=np.float64)
    out = np.empty(px.shape, dtype=np.uint8)
    oracle().trt_oracle_rgb8(px.ctypes.data, px.size // 3, out.ctypes.data)
    return out


@functools.lru_cache(maxsize=None)
def golden_meta():
    with open(os.path.join(GOLDEN, "golden.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def _frames():
    return dict(np.load(os.path.join(GOLDEN, "frames.npz")))


def read_ppm_bytes(raw):
    """Minimal P6 decode for test fixtures (the product loader is the C one in csrc/host)."""
    assert raw[:2] == b"P6"
    pos = 3
    while raw[pos:pos + 1] == b"#":
        pos = raw.index(b"\n", pos) + 1
    toks = []
    while len(toks) < 3:
        end = pos
        while raw[end:end + 1] not in (b" ", b"\n", b"\t", b"\r"):
            end += 1
        toks.append(int(raw[pos:end]))
        pos = end + 1
    w, h, mx = toks
    assert mx == 255
    return np.frombuffer(raw, dtype=np.uint8, count=w * h * 3, offset=pos).reshape(h, w, 3).copy()


def golden_ppm_raw(name, face):
    with open(os.path.join(GOLDEN, "skybox", name, face + ".ppm.z"), "rb") as fh:
        return zlib.decompress(fh.read())


@functools.lru_cache(maxsize=None)
def sky(name):
    if name == "synth":
        return np.load(os.path.join(GOLDEN, "synth_sky64.npz"))["sky"]
    return np.stack([read_ppm_bytes(golden_ppm_raw(name, f)) for f in FACES])


def golden_cases(size_classes=("small",)):
    return [c for c in golden_meta()["cases"] if c["size_class"] in size_classes]


def golden_scene(case):
    return S.SceneData.from_arrays(_frames(), sky(case["sky"]), prefix=case["name"] + "/")


def golden_fb(case):
    return _frames()[case["name"] + "/fb"] if case["has_fb"] else None


def bench_camera(width, height, t=1.0):
    """Stored reference camera at orbit time t (tests/golden/cameras.npz) with screen_width = 5*W/H."""
    d = np.load(os.path.join(GOLDEN, "cameras.npz"))
    i = int(np.argmin(np.abs(d["t"] - t)))
    assert abs(d["t"][i] - t) < 1e-12
    cam = d["camera"][i].copy()
    cam[13] = 5 * float(width) / float(height)
    return cam


@functools.lru_cache(maxsize=None)
def golden_full():
    """Full-size frames hashed by the genuine reference (tests/golden/make_golden_full.py): BASELINE configs 2-5 at the
    sizes the bench and the GPU tests render them, and frames with 1024^2 / 2048^2 cubemaps."""
    with open(os.path.join(GOLDEN, "golden_full.json")) as fh:
        return {c["name"]: c for c in json.load(fh)["cases"]}


def full_scene(case):
    """The scene of a golden_full case: SYNTH-v0 spheres, procedural cubemap, the reference's stored camera."""
    return S.synth_scene(case["spheres"], S.synth_sky(case["sky_dim"], seed=case["sky_seed"]),
                         np.array(case["camera"], dtype=np.float64), seed=case["scene_seed"])


def fuzz_scene(rng, w, h):
    """A random scene of the kinds kernels go wrong on: exact ties, nested and degenerate spheres, tilted and non-unit ground normals, lights on
    surfaces, cameras inside spheres and far away.  The fuzz tests share it; it draws from `rng` in a fixed order."""
    n = int(rng.choice([0, 1, 2, 5, 9, 31, 32, 33, 64, 65, 100]))
    sph = np.zeros((n, 9))
    if n:
        sph[:, :3] = rng.normal(size=(n, 3)) * rng.choice([0.5, 2.0, 6.0])
        sph[:, 3] = rng.uniform(0.05, 1.2, n) * rng.choice([0.3, 1.0, 2.0])
        sph[:, 4:7] = rng.uniform(0, 1, (n, 3))
        sph[:, 7] = rng.choice([0.0, 0.3, 0.9, 1.0], n)
        sph[:, 8] = 100.0
        if n >= 5:  # exact ties: duplicated spheres with different materials (first index must win), nested and degenerate ones
            sph[n // 2, :4] = sph[1, :4]
            sph[n - 1, :4] = sph[1, :4]
            sph[2, :3] = sph[3, :3]
            sph[2, 3] = sph[3, 3] * 0.5  # concentric, smaller: always hidden from outside
            sph[4, 3] = 0.0               # zero radius
    ground = S.demo_ground().copy()
    if rng.random() < 0.5:
        ground[0:3] = rng.normal(size=3)
        ground[3:6] = rng.normal(size=3) * rng.choice([1.0, 0.01, 30.0])  # non-unit normals too
    ground[9] = rng.choice([0.0, 0.2, 1.0])
    nd, npt = int(rng.integers(0, 3)), int(rng.integers(0, 4))
    dl = np.concatenate([rng.normal(size=(nd, 3)), rng.uniform(0, 1.2, (nd, 3))], axis=1)
    pl = np.concatenate([rng.normal(size=(npt, 3)) * 3, rng.uniform(0, 1.2, (npt, 3)), rng.uniform(0.1, 30, (npt, 1))], axis=1)
    if npt and n:
        pl[0, :3] = sph[0, :3] + np.array([0.0, sph[0, 3], 0.0])  # a light exactly on a sphere's surface
    cam = bench_camera(w, h, float(rng.choice([0.0, 0.5, 2.5, 10.0, 33.3])))
    if rng.random() < 0.3 and n:
        cam[9:12] = sph[0, :3] + 0.3 * sph[0, 3]  # camera inside a sphere
    if rng.random() < 0.3:
        cam[9:12] = rng.normal(size=3) * 20
    return S.SceneData(sph, ground, dl.reshape(-1, 6), pl.reshape(-1, 7), cam, sky("synth"))


# ---- the adversarial scene families: built here so that the GPU tests and tests/golden/make_golden_edges.py share them ----

def degenerate_scenes():
    base = S.synth_scene(24, sky("synth"), bench_camera(40, 24, 2.5), seed=3)

    def with_ground(point=None, normal=None, refl=None):
        g = base.ground.copy()
        if point is not None:
            g[0:3] = point
        if normal is not None:
            g[3:6] = normal
        if refl is not None:
            g[9] = g[14] = refl
        return S.SceneData(base.spheres, g, base.dir_lights, base.point_lights, base.camera, base.sky)

    out = [("ground without a normal", with_ground(normal=[0.0, 0.0, 0.0])),
           ("ground with a vanishing normal", with_ground(normal=[0.0, 1e-200, 0.0])),
           ("ground with a huge normal", with_ground(normal=[0.0, 1e150, 1e150], refl=1.0)),
           ("vertical mirror ground through the scene", with_ground(point=[0.3, 0.0, 0.0], normal=[1.0, 0.0, 0.0], refl=1.0))]
    cam = base.camera.copy()
    cam[10] = -2.0  # the eye exactly on the ground plane
    out.append(("eye on the ground plane", base.with_camera(cam)))
    cam = base.camera.copy()
    cam[9:12] = base.spheres[5, :3]  # the eye at a sphere's centre
    out.append(("eye at a sphere's centre", base.with_camera(cam)))
    sph = base.spheres.copy()
    sph[0, 3] = -0.4   # a negative radius (r*r is what the reference uses)
    sph[1, 3] = 0.0
    sph[2, :3] = [1e7, -3e6, 2e6]  # one sphere very far away: the tables' range explodes
    sph[3, :3] = sph[4, :3]        # concentric twins with equal radii: exact ties
    sph[3, 3] = sph[4, 3]
    out.append(("odd radii, a far sphere, exact twins", base.with_spheres(sph)))
    far = base.spheres.copy()
    far[:, :3] = far[:, :3] * 1e5  # an enormous scene: hit points lose digits against the 1e-6 nudge
    far[:, 3] *= 1e5
    gf = base.ground.copy()
    gf[1] *= 1e5
    cf = base.camera.copy()
    cf[9:12] *= 1e5
    out.append(("a scene 1e5 times larger", S.SceneData(far, gf, base.dir_lights, base.point_lights * np.array([1e5, 1e5, 1e5, 1, 1, 1, 1e10]), cf, base.sky)))
    pl = base.point_lights.copy()
    pl[0, :3] = base.camera[9:12]  # a light at the eye
    out.append(("a light at the eye", S.SceneData(base.spheres, base.ground, base.dir_lights, pl, base.camera, base.sky)))
    return out


def blocker_scene(w=96, h=54):
    """Ten point lights on, and within micrometres of, the surface of the demo sphere at (0,-1,0)."""
    base = S.demo_scene(sky("synth"), bench_camera(w, h))
    centre, radius = base.spheres[4, :3], base.spheres[4, 3]  # the sphere at (0,-1,0), just above the ground
    lights = []
    for k, eps in enumerate([0.0, 1e-6, -1e-6, 2e-6, -2e-6, 1.0000001e-6, 0.5e-6, -0.5e-6, 1e-5, -1e-5]):
        n = np.array([np.cos(0.7 * k), -0.8, np.sin(0.7 * k)])
        n /= np.linalg.norm(n)
        lights.append(list(centre + n * (radius + eps)) + [1.0, 0.9, 0.8, 3.0])
    return S.SceneData(base.spheres, base.ground, base.dir_lights, np.array(lights), base.camera, base.sky)


VALUE_SIZE = (48, 27)
VALUE_SHOTS = ((8, 3), (1, 1))  # (bounce limit, rays per pixel) of every value-domain scene
VALUE_DEEP = (12, 10)           # ... and of those whose reflectivities decide how long a path lives
# the scenes named for non-finite inputs: their frames must hold NaNs, from this bounce limit on.  A reflectivity is multiplied into
# the path's weight after the bounce's colour is taken (TRT.c:1035-1041), so at a bounce limit of 1 it cannot reach the frame.
NON_FINITE_VALUES = {"inf and NaN reflectivity": 2, "huge reflectivity": 2, "sphere colours out of range": 1}


def must_hold_nans(case_name, bounce_limit):
    parts = case_name.split("/")
    return parts[0] == "values" and bounce_limit >= NON_FINITE_VALUES.get(parts[1], 1 << 30)


def value_scenes():
    """[(name, scene, deep)]: material, light and camera values outside the domain every other scene stays in -- reflectivities at the
    END-round threshold, above one, negative, infinite, NaN and huge; light and sphere colours that are negative, huge, infinite or NaN;
    intensities that are negative, zero, huge, denormal-small or infinite; eyes so far out that the checker's (int) conversion overflows
    (2^31) or floor() is the identity (2^53).  `deep`: also rendered at VALUE_DEEP."""
    w, h = VALUE_SIZE
    base = S.synth_scene(24, sky("synth"), bench_camera(w, h, 2.5), seed=3)
    inf, nan = np.inf, np.nan

    def variant(refl=None, grefl=None, dcol=None, pcol=None, scol=None, eye=None, point_lights=None, ground_y=None):
        sph, g, dl = base.spheres.copy(), base.ground.copy(), base.dir_lights.copy()
        pl, cam = (base.point_lights if point_lights is None else point_lights).copy(), base.camera.copy()
        if refl is not None:
            sph[:, 7] = np.resize(refl, len(sph))
        if scol is not None:
            sph[:, 4:7] = np.resize(scol, (len(sph), 3))
        if grefl is not None:
            g[9], g[14] = grefl  # even, odd
        if dcol is not None:
            dl[:, 3:6] = np.resize(dcol, (len(dl), 3))
        if pcol is not None:
            pl[:, 3:6] = np.resize(pcol, (len(pl), 3))
        if eye is not None:
            cam[9:12] = eye
        if ground_y is not None:
            g[1] = ground_y
        return S.SceneData(sph, g, dl, pl, cam, base.sky)

    threshold = [1e-5, np.nextafter(1e-5, 1), np.nextafter(1e-5, 0), 0.003, 0.0032, 0.01, 0.05, 0.1, 1e-3, 0.99999]
    # five point lights, one intensity each; the last lies on the ground plane straight under the eye, so that the nudged ground hits
    # around it are a micrometre from it and its shadow rays run along the plane
    eye = base.camera[9:12]
    five = np.array([[0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0], [2.0, 3.0, -1.5, 0.9, 0.7, 0.3, 0.0], [-3.0, 0.5, 2.0, 0.2, 0.8, 0.9, 0.0],
                     [1.5, 1.0, 2.5, 0.6, 0.6, 0.9, 0.0], [eye[0], base.ground[1], eye[2], 1.0, 0.9, 0.8, 0.0]])
    five[:, 6] = np.resize([-1.0, 0.0, 1e308, 1e-300, inf], 5)
    return [("threshold reflectivities", variant(refl=threshold, grefl=(0.0031, 0.0033)), True),
            ("reflectivity above one", variant(refl=[1.5, 3.0, 1.0, 10.0], grefl=(2.0, 1.0)), False),
            ("negative reflectivity", variant(refl=[-0.5, 0.5, -1.0, 1.0], grefl=(-0.2, 0.2)), False),
            ("inf and NaN reflectivity", variant(refl=[inf, 0.5, nan, 1.0, -inf], grefl=(0.2, nan)), True),
            ("huge reflectivity", variant(refl=[1e200, 1e-200, 1e308], grefl=(1e160, 1e-160)), True),
            ("light colours out of range", variant(dcol=[-0.5, 2.0, 1e300], pcol=[5.0, -1e300, 0.5]), False),
            ("point-light intensities", variant(point_lights=five), False),
            ("sphere colours out of range", variant(scol=[[-1.0, 2.0, 1e300], [0.5, inf, -inf], [nan, 0.0, -0.0]]), False),
            ("checker beyond 2^31", variant(eye=[3e9, 5.0, -7e9]), False),
            ("checker beyond 2^53", variant(eye=[3e15, 5e3, -7e15]), False),
            # A ray's direction is the screen point minus the eye (TRT.c:1005): from the far eyes above every ray heads for the origin and
            # meets the checker, if at all, below -2^31, where x86-64's conversion and a saturating one agree (0x80000000).  Under a
            # ground 3e9 below the scene, rays of every direction come down on both sides of +-2^31: above +2^31 the reference's tile is
            # even (0x80000000) where a saturating conversion makes it odd (0x7fffffff).
            ("checker beyond 2^31 on a ground 3e9 below", variant(ground_y=-3e9), False),
            ("eye 1e6 above the ground", variant(eye=[0.5, 1e6, 0.25]), False)]


def non_finite_light_scene():
    """The value-domain base scene with a dim second directional light whose direction has a NaN component (normalize_vector leaves it
    alone) and a second point light infinitely far away (strength 0, direction inf/inf).  A light direction that is not a number is the
    only NaN operand fmin(n.l, 1.0) of TRT.c:911/945 can get; it answers 1.0, where a plain `1 < x ? 1 : x` would pass the NaN on.
    The reference itself is not defined here: such a shadow ray hits nothing, and its sky look-up then indexes CUBEMAP_AXES[-1]
    (TRT.c:703-717; the compiled reference ends in a segmentation fault on this scene).  So there is no recorded frame: the oracle,
    whose shadow rays look nothing up, is the judge, and fmin's answer is the C standard's."""
    w, h = VALUE_SIZE
    base = S.synth_scene(24, sky("synth"), bench_camera(w, h, 2.5), seed=3)
    dl = np.concatenate([base.dir_lights, [[np.nan, -1.0, -1.0, 0.3, 0.2, 0.1]]])
    pl = np.concatenate([base.point_lights, [[np.inf, 3.0, 0.0, 0.9, 0.7, 0.3, 10.0]]])
    return S.SceneData(base.spheres, base.ground, dl, pl, base.camera, base.sky)


# ---- the camera family: the base scene of the value-domain family under cameras outside the domain every other scene stays in ----
# (tests/test_camera_edges.py, tests/golden/make_golden_cameras.py; a family of its own, not part of edge_case_inputs)
CAMERA_BASE = "base"
CAMERA_WIDE = "twice the screen on twice the columns"
CAMERA_TRIO = ("trio/rolled", "trio/sheared", "trio/left-handed x3")
COS37, SIN37 = 0.7986355100472928, 0.6018150231520483  # literals: the recorded cameras do not hang on a libm


def _basis_variants(cam):
    """{name: basis[9]} of the camera family, from the orthonormal basis of `cam`"""
    x, y, z = cam[0:3].copy(), cam[3:6].copy(), cam[6:9].copy()
    cat = np.concatenate
    return {"x3": cat([x * 3.0, y * 3.0, z * 3.0]), "sheared": cat([x + 0.5 * y, y, z + 0.3 * x]), "left-handed": cat([-x, y, z]),
            "singular": cat([x, x, z]), "y = 0": cat([x, 0.0 * y, z]), "rolled 37 degrees": cat([COS37 * x + SIN37 * y, COS37 * y - SIN37 * x, z]),
            "all zero": np.zeros(9), "x1e-200": cat([x, y, z]) * 1e-200, "x1e200": cat([x, y, z]) * 1e200,
            "x = NaN": cat([np.full(3, np.nan), y, z]), "left-handed x3": cat([-x, y, z]) * 3.0}


def screen_point(cam, w, h, row, column):
    """the point of the screen that the first ray of pixel (row, column) goes through, in the operation order of TRT.c:987-1002 (numpy's
    float64 arithmetic is the reference's, one rounding per operation); where triangle_wave(0) == 0 that ray has no jitter"""
    sw, sh = np.float64(cam[13]), np.float64(cam[14])
    sx = (np.float64(column) / np.float64(w)) * sw - sw / np.float64(2.0)
    sy = -((np.float64(row) / np.float64(h)) * sh - sh / np.float64(2.0))
    sz = -np.float64(cam[12])
    p = np.zeros(3)
    p = p + cam[0:3] * sx
    p = p + cam[3:6] * sy
    return p + cam[6:9] * sz


def camera_scenes():
    """[(name, scene, w, h, defined)]: the base scene of value_scenes() under cameras that leave bench_camera()'s domain -- screen
    distances that are zero, negative, tiny, huge or not finite; screens that are empty, mirrored, tiny, huge or not finite; bases that
    are scaled, sheared, left-handed, singular, zero or not finite; eyes at the origin, a denormal away from it, not finite, or on the
    screen itself.  `defined`: every primary direction is finite and not of zero length, so the reference renders the camera (its two
    builds agree bit for bit); otherwise a sky look-up of the reference indexes outside its tables and the compiled reference dies
    (see non_finite_light_scene), and the library's own definitions apply (csrc/trt_device.hpp, sky_texel)."""
    w, h = VALUE_SIZE
    base = S.synth_scene(24, sky("synth"), bench_camera(w, h, 2.5), seed=3)
    bases = _basis_variants(base.camera)
    inf, nan = np.inf, np.nan
    out = []

    def case(name, defined, size=(w, h), **fields):
        cam = base.camera.copy()
        cam[13] = 5 * float(size[0]) / float(size[1])
        for key, value in fields.items():
            cam[{"basis": slice(0, 9), "eye": slice(9, 12), "sd": 12, "sw": 13, "sh": 14}[key]] = value
        out.append((name, base.with_camera(cam), size[0], size[1], defined))
        return cam

    sw = base.camera[13]
    case(CAMERA_BASE, True)
    for v in (0.0, -0.0, -1.0, 1e-300, 0.05, 40.0):
        case(f"screen_distance {v!r}", True, sd=v)
    case("screen_width 0", True, sw=0.0)
    case("screen_height 0", True, sh=0.0)
    case("screen_width negated", True, sw=-sw)
    case("screen_height -5", True, sh=-5.0)
    case("screen 1e-9", True, sw=1e-9, sh=1e-9)
    case("screen 1e9", True, sw=1e9, sh=1e9)
    case("screen_width 5e-324, screen_height 1e-310", True, sw=5e-324, sh=1e-310)
    for key in ("x3", "sheared", "left-handed", "singular", "y = 0", "rolled 37 degrees", "all zero", "x1e-200"):
        case(f"basis {key}", True, basis=bases[key])
    case("eye at the origin", True, eye=0.0)
    case("eye at the origin, screen_distance 0", True, eye=0.0, sd=0.0)
    case("eye at the origin, identity basis", True, eye=0.0, basis=np.eye(3).ravel())
    case("eye a denormal from the origin", True, eye=[1e-300, -1e-300, 1e-310])
    # the same pixel width as the base case (the jitter table is legitimately reused) on other axes
    case(CAMERA_WIDE, True, size=(2 * w, h), sw=2.0 * sw)
    # three cameras that share one odd screen, what a batch needs; a basis and an eye each
    eye = base.camera[9:12]
    for name, key, at in zip(CAMERA_TRIO, ("rolled 37 degrees", "sheared", "left-handed x3"),
                             (eye, eye + np.array([0.4, 0.3, -0.2]), eye * np.array([-1.25, 0.5, 1.5]))):
        case(name, True, sd=0.05, sw=-sw, sh=3.0, basis=bases[key], eye=at)
    # ---- not defined by the reference ----
    for v in (1e160, 1e300, inf, nan):
        case(f"screen_distance {v!r}", False, sd=v)
    case("screen_width inf", False, sw=inf)
    case("screen_height NaN", False, sh=nan)
    case("screen 1e308", False, sw=1e308, sh=1e308)
    case("basis x1e200", False, basis=bases["x1e200"])
    case("basis x = NaN", False, basis=bases["x = NaN"])
    case("eye with a NaN component", False, eye=[eye[0], nan, eye[2]])
    case("eye with an infinite component", False, eye=[-inf, eye[1], eye[2]])
    case("eye 1e200 away", False, eye=[1e200, 1e200, -1e200])
    # a primary ray of zero length, at 48x28, where triangle_wave(0) == 0 leaves the first ray of a pixel on the pixel's own point
    tall = base.camera.copy()
    tall[13] = 5 * 48.0 / 28.0
    case("eye on the screen point of a pixel", False, size=(48, 28), eye=screen_point(tall, 48, 28, 9, 31))
    case("identity basis, eye at the origin, screen_distance 0", False, size=(48, 28), basis=np.eye(3).ravel(), eye=0.0, sd=0.0)
    assert len({n for n, *_ in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def camera_meta():
    with open(os.path.join(GOLDEN, "golden_camera_edges.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def _camera_edges():
    return dict(np.load(os.path.join(GOLDEN, "camera_edges.npz")))


def camera_cases():
    """the defined cases of the record, one per camera and shot: the keys of an edge case, and "camera": the camera's name"""
    return camera_meta()["cases"]


def camera_case_scene(case):
    """the scene the reference rendered: the family's base scene and the camera's fifteen doubles, both from the record"""
    a = _camera_edges()
    scene = unpack_scene(a["scene"], case["spheres"], case["dir_lights"], case["point_lights"])
    return scene.with_camera(a[case["scene"]])


def camera_fb(case):
    """the reference's double framebuffer [h, w, 3] (read-only), or None where only its hash is recorded"""
    if case["fb"] is None:
        return None
    fb = _camera_edges()[case["fb"]]
    fb.flags.writeable = False
    return fb


def assert_is_the_recorded_frame(got, case, want, positions_from, who):
    """A frame equals the record when its NaNs sit in the same places, every other value has the same bits, the counts of NaN and
    infinite values are the recorded ones and the FNV of the frame with its NaNs made one NaN is the recorded hash.  `want`: the
    recorded frame, or None where the archive keeps the case's hash only; then `positions_from` -- the oracle's frame, which the CPU
    test of the same case pins to that hash -- says where the NaNs and the values are."""
    if want is None:
        want = positions_from
    assert got.shape == want.shape == (case["h"], case["w"], 3)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (case["name"], who, "NaNs in other places", int((np.isnan(got) != np.isnan(want)).sum()))
    there = ~np.isnan(want)
    differ = bits(got)[there] != bits(want)[there]
    assert not differ.any(), (case["name"], who, "values differ", int(differ.sum()), np.argwhere(bits(got) != bits(want))[:4].tolist())
    assert (int(np.isnan(got).sum()), int(np.isinf(got).sum())) == (case["nan"], case["inf"]), (case["name"], who)
    assert fnv(canonical_nans(got)) == case["fb_fnv"], (case["name"], who)


def fuzz_case(seed):
    """(scene, w, h, bounce limit, rays per pixel) of fuzz seed `seed`, with the draws test_fuzzed_scenes_match_the_oracle makes"""
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(8, 72)), int(rng.integers(4, 40))
    b, spp = int(rng.integers(1, 9)), int(rng.choice([1, 3, 10]))
    return fuzz_scene(rng, w, h), w, h, b, spp


def edge_case_inputs():
    """Every case of tests/golden/golden_edges.json as its builder makes it: [(name, family, scene key, scene, w, h, b, spp)].  The
    frames of one scene at several (b, spp) share the scene key, under which edges.npz holds the scene's arrays once."""
    out = []
    for name, scene in degenerate_scenes():
        out.append((f"degenerate/{name}", "degenerate", f"degenerate/{name}", scene, 40, 24, 6, 3))
    for seed in range(12):
        scene, w, h, b, spp = fuzz_case(seed)
        out.append((f"fuzz/{seed}", "fuzz", f"fuzz/{seed}", scene, w, h, b, spp))
    out.append(("blocker/lights at blocker distance", "blocker", "blocker/lights at blocker distance", blocker_scene(), 96, 54, 4, 10))
    for name, scene, deep in value_scenes():
        for b, spp in VALUE_SHOTS + ((VALUE_DEEP,) if deep else ()):
            out.append((f"values/{name}/b{b}_s{spp}", "values", f"values/{name}", scene, *VALUE_SIZE, b, spp))
    return out


@functools.lru_cache(maxsize=None)
def edge_meta():
    with open(os.path.join(GOLDEN, "golden_edges.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def _edges():
    return dict(np.load(os.path.join(GOLDEN, "edges.npz")))


def edge_cases():
    return edge_meta()["cases"]


def edge_scene(case):
    """the scene the reference rendered, from the record kept with its frame"""
    return unpack_scene(_edges()[case["scene"]], case["spheres"], case["dir_lights"], case["point_lights"])


def pack_scene(scene):
    """one float64 record per scene (an archive member costs more than a small scene's arrays do): spheres, ground, lights, camera"""
    return np.concatenate([scene.spheres.ravel(), scene.ground, scene.dir_lights.ravel(), scene.point_lights.ravel(), scene.camera])


def unpack_scene(flat, spheres, dir_lights, point_lights):
    cuts = np.cumsum([9 * spheres, 16, 6 * dir_lights, 7 * point_lights, 15])
    assert flat.size == cuts[-1]
    sph, ground, dl, pl, cam = np.split(flat, cuts[:-1])
    return S.SceneData(sph, ground, dl, pl, cam, sky("synth"))


def edge_fb(case):
    """the reference's double framebuffer [h, w, 3] (read-only), or None where only its hash is recorded"""
    if case["fb"] is None:
        return None
    fb = _edges()[case["fb"]]  # frames that are equal bit for bit are held once
    fb.flags.writeable = False
    return fb


def canonical_nans(pixels):
    """a copy with every NaN replaced by one quiet NaN: x86-64 and the GPU make different default NaNs, hashes are taken of this"""
    out = np.array(pixels, dtype=np.float64)
    out[np.isnan(out)] = np.float64("nan")
    return out


# ---- the render kernels the GPU parity tests go through ----
# the production kernel as it ships (the shading decoupled from the owning lane for scenes of three lights or more,
# trt_set_compaction(-1)), the same with the decoupling forced on, and the reference-order kernel -- an independent HIP
# implementation of the path
COMPACT = "production_rounds_compact"
PLAIN = "production_rounds_plain"  # the decoupling forced off (what ships for scenes of one or two lights)
KERNELS = [hip.Context.PRODUCTION, COMPACT, hip.Context.REFERENCE_ORDER]
KERNEL_IDS = ["production_rounds", COMPACT, "reference_order"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def render(ctx, scene, w, h, b, s, kernel=hip.Context.PRODUCTION, rows=None):
    ctx.set_kernel(hip.Context.PRODUCTION if kernel in (COMPACT, PLAIN) else kernel)
    ctx.set_compaction({COMPACT: 1, PLAIN: 0}.get(kernel, -1))
    ctx.set_scene(scene)
    return ctx.render_host(scene.camera, rows or hip.RowSet.whole(w, h), b, s)


# ---- directed scenes of tests/test_candidate_edges.py: every ray's answer hangs on ONE known sphere at a known place of the sweep or of a list ----

def index_colour(i):
    """a colour that names sphere i (the probe returns the winner's material): three exactly representable components"""
    return np.array([(i % 16 + 1) / 32.0, ((i // 16) % 16 + 1) / 32.0, (i // 256 + 1) / 32.0])


def directed_spheres(centres, radii):
    centres, radii = np.asarray(centres, dtype=np.float64).reshape(-1, 3), np.asarray(radii, dtype=np.float64).ravel()
    sph = np.zeros((len(centres), 9))
    sph[:, :3], sph[:, 3] = centres, radii
    for i in range(len(sph)):
        sph[i, 4:7] = index_colour(i)
    sph[:, 7], sph[:, 8] = 0.3, 100.0
    return sph


def oracle_probe(scene, rays):
    """what trt_oracle_trace_ray and trt_oracle_apply_lighting answer for every ray, in the probes' layout"""
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    sc, lib, n = scene.as_scene(), oracle(), len(rays)
    out = {"obj": np.zeros(n, dtype=np.int32), "point": np.zeros((n, 3)), "normal": np.zeros((n, 3)), "material": np.zeros((n, 5)), "lit": np.zeros((n, 3))}
    for i in range(n):
        ray = L.Ray.from_buffer(rays[i])
        pt, nr, mt = L.Vector(), L.Vector(), L.Material()
        obj = lib.trt_oracle_trace_ray(C.byref(sc), C.byref(ray), C.byref(pt), C.byref(nr), C.byref(mt))
        out["obj"][i] = obj
        out["point"][i], out["normal"][i] = (pt.x, pt.y, pt.z), (nr.x, nr.y, nr.z)
        out["material"][i] = (mt.color.x, mt.color.y, mt.color.z, mt.reflectivity, mt.specularity)
        if obj != L.NONE:
            lib.trt_oracle_apply_lighting(C.byref(sc), C.byref(pt), C.byref(nr), C.byref(mt), None)
            out["lit"][i] = (mt.color.x, mt.color.y, mt.color.z)
    return out


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt(v @ v)


SWEEP_COUNTS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 200)
SWEEP_TWINS = ("ends", (31, 32), (63, 64), (62, 65))  # (i, j): sphere j repeats sphere i; "ends": (0, n - 1)
# light travel directions at most 27 degrees off the vertical, point lights high above the layer: a line from a light through a sphere's centre
# leaves the layer of spheres (2.4 thick) within 0.9 of that centre sideways, and the next sphere is 2.4 away
SWEEP_DIR_LIGHTS = np.array([[-0.3, -1.0, -0.2, 0.15, 0.1, 0.05], [0.4, -1.0, 0.1, 0.05, 0.15, 0.1], [0.1, -1.0, -0.5, 0.1, 0.05, 0.15]])
SWEEP_POINT_LIGHTS = np.array([[4.0, 40.0, -3.0, 0.15, 0.15, 0.05, 1500.0], [-6.0, 45.0, 5.0, 0.05, 0.1, 0.15, 1700.0]])


def sweep_scene(n, n_dir=3, n_point=2, twins=()):
    """n spheres in one layer on a lattice of pitch 3 (radii 0.3 .. 0.6, centres 2.7 .. 3.3 above the ground), lit from above"""
    cols = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    off = 1.5 * (cols - 1)
    centres = np.stack([3.0 * (k % cols) - off, 1.0 + 0.15 * ((k * 7) % 5 - 2), 3.0 * (k // cols) - off], axis=1)
    radii = 0.3 + 0.05 * ((k * 5) % 7)
    for i, j in twins:
        centres[j], radii[j] = centres[i], radii[i]
    return S.SceneData(directed_spheres(centres, radii), S.demo_ground(), SWEEP_DIR_LIGHTS[:n_dir], SWEEP_POINT_LIGHTS[:n_point],
                       bench_camera(40, 24), sky("synth"))


def sweep_twins(n):
    return [(0, n - 1) if t == "ends" else t for t in SWEEP_TWINS if (n >= 2 if t == "ends" else t[1] < n)]


def sweep_sphere_rays(scene):
    """(rays, wanted sphere or -1): ray i starts 0.4 outside sphere i and runs at its centre; then rays that meet the sky and the ground between the
    spheres; then rays whose direction is not of unit length (the sweep then proposes EVERY sphere of a chunk, padding included)"""
    sph, n = scene.spheres, len(scene.spheres)
    rays, want = [], []
    for i in range(n):
        u = _unit([np.cos(0.7 * i), 0.8, np.sin(0.7 * i)])
        rays.append(np.concatenate([sph[i, :3] + (sph[i, 3] + 0.4) * u, -u]))
        want.append(i)
    top = sph[:, 1].max() + 4.0
    for q in range(4):
        rays.append(np.concatenate([[sph[q % n, 0] + 1.5, top, sph[q % n, 2] + 1.5], _unit([0.3 * q - 0.4, 1.0, 0.2])]))  # sky
        rays.append(np.concatenate([[sph[(5 * q) % n, 0] + 1.5, top, sph[(5 * q) % n, 2] + 1.5], [0.0, -1.0, 0.0]]))       # ground, between spheres
        want += [-1, -1]
    for q, i in enumerate(sorted({0, n // 2, n - 1, (n - 1) // 8 * 8, max(n - 2, 0)})):
        scale = (2.0, 0.5, 3.0, 1.0 + 1e-9, 0.25)[q]
        rays.append(np.concatenate([sph[i, :3] + np.array([0.0, sph[i, 3] + 0.4, 0.0]), [0.0, -scale, 0.0]]))
        want.append(i)
    rays.append(np.concatenate([[sph[0, 0] + 1.5, top, sph[0, 2] + 1.5], [0.6, 2.0, 0.2]]))    # not of unit length, and nothing hit: sky
    rays.append(np.concatenate([[sph[0, 0] + 1.5, top, sph[0, 2] + 1.5], [0.0, -0.5, 0.0]]))  # ... the ground
    want += [-1, -1]
    return np.array(rays), np.array(want)


def sweep_shadow_rays(scene):
    """(rays, light, sphere): probe rays straight down onto ground points; from point (light l, sphere i) the centre of sphere i -- and no other
    sphere -- stands between the point and light l (sphere -1: points well outside the lattice that nothing shadows)"""
    sph, gy = scene.spheres, scene.ground[1]
    rays, light, sphere = [], [], []
    nd = len(scene.dir_lights)
    for l in range(nd + len(scene.point_lights)):
        for i in range(len(sph)):
            c = sph[i, :3]
            along = scene.dir_lights[l, :3] if l < nd else c - scene.point_lights[l - nd, :3]  # the way the light travels through the centre
            g = c + along * ((gy - c[1]) / along[1])
            rays.append([g[0], gy + 0.05, g[2], 0.0, -1.0, 0.0])
            light.append(l), sphere.append(i)
    far = np.abs(sph[:, [0, 2]]).max() + 8.0
    for q in range(6):
        rays.append([far + 2.0 * q, gy + 0.05, (far + 1.0 * q) * (-1.0 if q & 1 else 1.0), 0.0, -1.0, 0.0])
        light.append(-1), sphere.append(-1)
    return np.array(rays), np.array(light), np.array(sphere)


def without_sphere(scene, i):
    return scene.with_spheres(np.delete(scene.spheres, i, axis=0))


# (c), (d): a CLUSTER of K spheres inside one table cell, seen from an apex (the eye; a point light; a ground point looking at a directional
# light) along the cell's middle direction: `s` of them on the ray's line -- the nearest at list position p --, the others 1.2 .. 1.65 off the line
# (radius 0.25: the FP32 filter rejects them).  List positions are ascending sphere indices: position k of the returned arrays.
def cluster(apex, direction, K, s, p, twin=None):
    d = _unit(direction)
    e1 = _unit(np.cross(d, [0.0, 0.0, 1.0] if abs(d[2]) < 0.9 else [1.0, 0.0, 0.0]))
    e2 = np.cross(d, e1)
    on = [p]  # list positions on the line, nearest first: p, then from both ends of the list inwards
    for k in (k for pair in zip(range(K), range(K - 1, -1, -1)) for k in pair):
        if k not in on:
            on.append(k)
    on = on[:s]
    centres = np.zeros((K, 3))
    m = 0
    for k in range(K):
        if k in on:
            centres[k] = apex + d * (12.0 + 1.5 * on.index(k))
        else:
            phi = 2.4 * m
            centres[k] = apex + d * (14.0 + 0.5 * (m % 9)) + (1.2 + 0.15 * (m % 4)) * (np.cos(phi) * e1 + np.sin(phi) * e2)
            m += 1
    if twin:  # the second of the pair repeats the first, which is the nearest on the line
        centres[twin[1]] = centres[twin[0]]
    return centres, np.full(K, 0.25)


WIDE_LOW = 3      # 16-bit entries: the cluster's first list position is this sphere, the others start at WIDE_FROM
WIDE_FROM = 300


def place_cluster(parts, wide, total=None):
    """the numbering of a directed scene: parts = [(centres, radii)]; the first part's list positions 0 .. K - 1 become sphere 0 .. K - 1 (8-bit
    entries) or WIDE_LOW, WIDE_FROM .. (16-bit), the other parts follow.  Returns ([sphere indices of each part], number of spheres of the
    scene: at least `total`, more than 256 for 16-bit entries); the caller places the parts and fills the indices left over"""
    K = len(parts[0][0])
    first = ([WIDE_LOW] + list(range(WIDE_FROM, WIDE_FROM + K - 1))) if wide else list(range(K))
    nxt = max(max(first) + 1, WIDE_FROM if wide else 0)  # 16-bit entries: more than 256 spheres whatever K is
    index = [first]
    for c, _ in parts[1:]:
        index.append(list(range(nxt, nxt + len(c))))
        nxt += len(c)
    return index, max(nxt, total or 0)


EYE = np.array([0.0, 1.0, -20.0])
EYE_MAIN, EYE_SHORT, EYE_OVER = np.array([-0.25, 0.25, 1.0]), np.array([1.0, 0.25, -0.25]), np.array([-1.0, 0.25, 0.25])  # cell middles of a 4-cell face
OVER_COUNT = 13  # a list longer than the prefilter's threshold, all of it on the ray: more survivors than the compaction holds


def eye_list_scene(K, s, p, wide, twin=None):
    """(scene, {"main", "short", "over"}: ray from the eye into the cell) for the eye's table at set_path_grids(4, 3): the directed cluster in one
    cell, one sphere in a second cell, OVER_COUNT spheres in a row in a third; 16-bit entries: 300 + spheres, the fillers behind the eye"""
    parts = [cluster(EYE, EYE_MAIN, K, s, p, twin), cluster(EYE, EYE_SHORT, 1, 1, 0), cluster(EYE, EYE_OVER, OVER_COUNT, OVER_COUNT, 0)]
    index, n = place_cluster(parts, wide)
    centres, radii = np.zeros((n, 3)), np.full(n, 0.1)
    taken = np.zeros(n, dtype=bool)
    for (c, r), idx in zip(parts, index):
        centres[idx], radii[idx], taken[idx] = c, r, True
    free = np.nonzero(~taken)[0]
    q = np.arange(len(free))
    centres[free] = EYE + np.stack([1.2 * (q % 18) - 10.0, 1.2 * (q // 18) + 2.0, np.full(len(q), -40.0)], axis=1)  # a wall behind the eye
    cam = bench_camera(24, 16)
    cam[9:12] = EYE
    d, pl = S.demo_lights()
    scene = S.SceneData(directed_spheres(centres, radii), S.demo_ground(), d * np.array([1, 1, 1, 0.3, 0.3, 0.3]), pl * np.array([1, 1, 1, 0.3, 0.3, 0.3, 60.0]),
                        cam, sky("synth"))
    rays = {k: np.concatenate([EYE, _unit(v)]) for k, v in (("main", EYE_MAIN), ("short", EYE_SHORT), ("over", EYE_OVER))}
    return scene, rays, index[0]


FAMILY_SOURCE = np.array([0.0, 4.0, 0.0])  # the sphere (radius 0.25, the scene's LAST index) the rays of a sphere's families start on
# per role: the ray's direction -- the middle of a cell of a 3-cell face -- and where on the source sphere it (kind "sphere") or its parent (kind
# "mirror") starts: well inside a patch for 1 and 2 patch cells per face side
FAMILY_RAYS = {"sphere": {"main": ([0.0, 0.0, 1.0], [0.4, 0.3, 1.0]), "short": ([1.0, 0.0, 0.0], [1.0, 0.3, 0.4]), "over": ([-1.0, 0.0, 0.0], [-1.0, 0.3, 0.4])},
               "mirror": {"main": ([0.0, 2.0 / 3.0, 1.0], [0.4, -2.0 / 3.0, 1.0]), "short": ([1.0, 2.0 / 3.0, 0.0], [1.0, -2.0 / 3.0, 0.4]),
                          "over": ([-1.0, 2.0 / 3.0, 0.0], [-1.0, -2.0 / 3.0, 0.4])}}
FAMILY_CASES = ((5, 1, 4), (9, 1, 8), (16, 4, 7), (16, 10, 8))  # (K, s, p) of the cluster: inline, pooled, prefiltered and compacted, prefiltered and overflowing


def family_list_scene(kind, K, s, p):
    """(scene, {"main", "short", "over"}: ray, the same: origin on the source sphere that names the patch, the cluster's sphere indices, the source's
    index) for the tables of ONE sphere's families at set_path_grids(4, 3).  kind "sphere": the rays start on the source sphere; "mirror": they start on
    the ground, where a ray from the source sphere was reflected.  Along the main ray a cluster as in eye_list_scene, along the others one sphere and
    OVER_COUNT spheres in a row"""
    ground = S.demo_ground()
    gy, r = ground[1], 0.25
    assert np.array_equal(ground[3:6], [0.0, 1.0, 0.0])
    rays, starts, parts = {}, {}, []
    for role, (Kc, sc, pc) in (("main", (K, s, p)), ("short", (1, 1, 0)), ("over", (OVER_COUNT, OVER_COUNT, 0))):
        d, w = (_unit(v) for v in FAMILY_RAYS[kind][role])
        o = FAMILY_SOURCE + r * w
        starts[role] = o
        if kind == "mirror":  # the parent leaves o downwards, with d's mirror image, and meets the ground at g
            dp = d * np.array([1.0, -1.0, 1.0])
            g = o + dp * ((gy - o[1]) / dp[1])
            o = np.array([g[0], gy + 1e-6, g[2]])
        rays[role] = np.concatenate([o, d])
        parts.append(cluster(o, d, Kc, sc, pc))
    parts.append((FAMILY_SOURCE[None, :], np.array([r])))
    index, n = place_cluster(parts, False)
    centres, radii = np.zeros((n, 3)), np.zeros(n)
    for (c, rr), idx in zip(parts, index):
        centres[idx], radii[idx] = c, rr
    cam = bench_camera(24, 16)
    cam[9:12] = EYE + np.array([0.0, 0.0, -40.0])
    d, pl = S.demo_lights()
    scene = S.SceneData(directed_spheres(centres, radii), ground, d * np.array([1, 1, 1, 0.3, 0.3, 0.3]), pl * np.array([1, 1, 1, 0.3, 0.3, 0.3, 60.0]), cam, sky("synth"))
    return scene, rays, starts, index[0], index[3][0]


def list_cases(wide):
    """[(K, s, p)]: list lengths either side of inline / pooled / prefiltered and of a pool word; the nearest sphere first, last, and either side of a
    pool-word boundary; for prefiltered lists (K > 12) survivors 1, the compaction's capacity, one more, all"""
    per = 4 if wide else 8
    out = []
    for K in ((1, 3, 4, 5, 8, 9, 12, 13, 16, 17) if wide else (1, 7, 8, 9, 12, 13, 16, 17, 24, 25)):
        for p in sorted({0, K - 1, per - 1, per} & set(range(K))):
            for s in ((1, per, per + 1, K) if K > 12 else sorted({1, K})):
                out.append((K, s, p))
    return out


def wave_layouts(rays, lane):
    """two waves of 64 probe rays: the directed ray in lane `lane` among short-list neighbours; the same among neighbours whose long lists overflow the
    prefilter's compaction"""
    out = np.concatenate([np.tile(rays["short"], (64, 1)), np.tile(rays["over"], (64, 1))])
    out[lane], out[64 + lane] = rays["main"], rays["main"]
    return out


POINT_LIGHT = np.array([0.0, 30.0, 0.0])
POINT_MAIN, POINT_EMPTY, POINT_OVER = np.array([-0.5, -1.0, 0.5]), np.array([0.5, -1.0, -0.5]), np.array([0.5, -1.0, 0.5])  # cell middles of a 2-cell face of the light's cube map
DIR_TRAVEL = np.array([0.3, -1.0, 0.2])


def _dir_basis(to_light):
    """the plane basis trt_dirgrid_prepare makes across a light direction"""
    d = _unit(to_light)
    t = np.zeros(3)
    t[int(np.argmin(np.abs(d)))] = 1.0
    e1 = _unit(np.cross(d, t))
    return d, e1, np.cross(d, e1)


def light_list_scene(kind, K, p, wide, unsure=False, total=None):
    """(scene, {"main", "other", "over"}: probe rays onto ground points, sphere index of every list position) for ONE light's table at
    set_light_grids(8, 2), set_light_slabs(1, 1).  kind 0: a directional light; 1: a point light.  From the main ground point the shadow ray's cell lists
    the K spheres of a cluster, of which the one at list position p blocks the light.  From "other" the cell is empty; from "over" it lists OVER_COUNT
    spheres in a row towards the light: a long list all of which the prefilter keeps.  unsure (point light): nothing of the cluster blocks; one more sphere, of the
    highest index, lies behind the light with its surface through it: a hit as far as the light, which the any-hit search cannot decide"""
    gy = S.demo_ground()[1]
    if kind == 1:
        o = POINT_LIGHT + POINT_MAIN * ((gy - POINT_LIGHT[1]) / POINT_MAIN[1])
        other = POINT_LIGHT + POINT_EMPTY * ((gy - POINT_LIGHT[1]) / POINT_EMPTY[1])
        over = POINT_LIGHT + POINT_OVER * ((gy - POINT_LIGHT[1]) / POINT_OVER[1])
        parts = [cluster(POINT_LIGHT, POINT_MAIN, K, 0 if unsure else 1, p), cluster(POINT_LIGHT, POINT_OVER, OVER_COUNT, OVER_COUNT, 0)]
        if unsure:
            u = _unit(POINT_LIGHT - o)
            parts.append((np.array([POINT_LIGHT + u * 0.5]), np.array([0.5])))
    else:
        d, e1, e2 = _dir_basis(-DIR_TRAVEL)
        frame = [np.array([0.0, 10.0, 0.0]) + 50.0 * (a * e1 + b * e2) for a, b in ((-1, -1), (1, 1))]  # two far spheres size the grid: cells of 25
        q = np.array([0.0, 10.0, 0.0]) + 12.5 * (e1 + e2)                    # the middle of a cell
        o = q + DIR_TRAVEL * ((gy - q[1]) / DIR_TRAVEL[1])
        q2 = np.array([0.0, 10.0, 0.0]) + 12.5 * (e1 - e2)                   # another, empty, cell
        other = q2 + DIR_TRAVEL * ((gy - q2[1]) / DIR_TRAVEL[1])
        q3 = np.array([0.0, 10.0, 0.0]) + 12.5 * (e2 - e1)                   # a third cell: a row of spheres towards the light
        over = q3 + DIR_TRAVEL * ((gy - q3[1]) / DIR_TRAVEL[1])
        parts = [cluster(o, d, K, 1, p), (np.array(frame), np.array([0.25, 0.25])), cluster(over, d, OVER_COUNT, OVER_COUNT, 0)]
    index, n = place_cluster(parts, wide, total)
    centres, radii = np.zeros((n, 3)), np.full(n, 0.1)
    taken = np.zeros(n, dtype=bool)
    for (c, r), idx in zip(parts, index):
        centres[idx], radii[idx], taken[idx] = c, r, True
    free = np.nonzero(~taken)[0]
    k = np.arange(len(free))
    side = int(np.ceil(np.sqrt(max(len(free), 1))))
    if kind == 1:  # fillers above the light: other faces of its cube map
        centres[free] = POINT_LIGHT + np.stack([1.2 * (k % side) - 0.6 * side, np.full(len(k), 15.0), 1.2 * (k // side) - 0.6 * side], axis=1)
    else:          # fillers over the middle of another cell of the grid
        centres[free] = np.array([0.0, 10.0, 0.0]) - 12.5 * (e1 + e2) + np.outer(20.0 / side * (k % side) - 10.0, e1) + np.outer(20.0 / side * (k // side) - 10.0, e2)
    dl = np.array([[*DIR_TRAVEL, 0.5, 0.4, 0.3]]) if kind == 0 else np.zeros((0, 6))
    pl = np.array([[*POINT_LIGHT, 0.5, 0.4, 0.3, 900.0]]) if kind == 1 else np.zeros((0, 7))
    scene = S.SceneData(directed_spheres(centres, radii), S.demo_ground(), dl, pl, bench_camera(24, 16), sky("synth"))
    rays = {k: np.array([v[0], gy + 0.05, v[2], 0.0, -1.0, 0.0]) for k, v in (("main", o), ("other", other), ("over", over))}
    return scene, rays, index[0]


# ---- the scaffold of the tests of the whole-frame outputs: the orbit's cameras, device buffers with guards, byte-for-byte comparisons ----

GUARD = 64   # bytes of 0xA5 either side of every device byte buffer
STORE = 4    # the widest store a text pass uses: an aligned 32-bit word


def anim_cameras(indices, w, h):
    d = np.load(os.path.join(GOLDEN, "cameras_anim.npz"))
    cams = d["camera"][list(indices)].copy()
    cams[:, 13] = 5 * float(w) / float(h)
    return cams


def owned_rows(rows):
    return hip.lib().trt_rowset_rows(C.byref(rows))


class DeviceBytes:
    """n bytes of device memory that start `offset` bytes behind a 4-aligned address, GUARD bytes of 0xA5 in front and behind; the n bytes
    themselves hold 0xA5 too, or, `raw`, whatever the allocation held"""

    def __init__(self, n, offset=0, raw=False):
        import torch
        self.n, self.start = n, GUARD + offset
        size = GUARD + STORE + n + GUARD
        if raw:
            self.buf = torch.empty(size, dtype=torch.uint8, device="cuda:0")
            self.buf[:self.start] = 0xA5
            self.buf[self.start + n:] = 0xA5
        else:
            self.buf = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert self.buf.data_ptr() % STORE == 0 and GUARD % STORE == 0
        torch.cuda.synchronize()  # the fill is on torch's stream, the render on the context's

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    def read(self, ctx, what=""):
        """the n bytes, once every byte outside them has been seen unchanged"""
        ctx.synchronize()
        got = self.buf.cpu().numpy()
        outside = np.concatenate([got[:self.start], got[self.start + self.n:]])
        assert outside.size >= 2 * GUARD and (outside == 0xA5).all(), f"{what}: {int((outside != 0xA5).sum())} bytes outside the {self.n} were written"
        return got[self.start:self.start + self.n].copy()

    def untouched(self, ctx):
        ctx.synchronize()
        return bool((self.buf.cpu().numpy() == 0xA5).all())


def same_text(got, want, what, whose="the emitter's"):
    """uint8 arrays of one shape, byte for byte"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    wrong = got != want
    if wrong.any():
        at = int(np.argmax(wrong.reshape(-1)))
        raise AssertionError(f"{what}: {int(wrong.sum())} of {wrong.size} bytes differ from {whose}, the first at {at}: "
                             f"{bytes(got.reshape(-1)[max(at - 8, 0):at + 8])!r} for {bytes(want.reshape(-1)[max(at - 8, 0):at + 8])!r}")


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    wrong = got != want
    assert not wrong.any(), f"{what}: {int(wrong.sum())} of {wrong.size} bytes differ from the oracle's, the first at {int(np.argmax(wrong.reshape(-1)))}"
