"""The loader of tests/specular_restatement.c -- the CPU restatement of the frame producer with the specular extension (checker only) --
and what the specular tests share of its answers: frames, ray counts, the log of every (hit, light) term, single shaded rays."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import support as T
from terminalraytracer_amd import layout as L
from terminalraytracer_amd import scenes as S

# the columns of a logged term (specular_restatement.c, TERM_*)
D, NORMAL, LIGHT_DIR, INTENSITY, COLOUR, E, POINT, MATERIAL, SPEC, TERM_DOUBLES = slice(0, 3), slice(3, 6), slice(6, 9), 9, slice(10, 13), 13, 14, slice(15, 18), slice(18, 21), 21


class Stats(C.Structure):
    _fields_ = [("path_rays", C.c_ulonglong), ("shadow_rays", C.c_ulonglong)]


class Log(C.Structure):
    _fields_ = [("terms", C.c_void_p), ("capacity", C.c_size_t), ("count", C.c_size_t)]


@functools.lru_cache(maxsize=None)
def restatement():
    """tests/specular_restatement.c compiled for the host, the way support.lightgrid_checker() compiles its checker"""
    so = T.checker_so("libspecularrestatement")
    src = os.path.join(T.ROOT, "tests", "specular_restatement.c")
    inc = os.path.join(T.ROOT, "include")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(inc, "trt.h")))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared"] + T.CHECKER_FLAGS + ["-I" + inc, "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    lib.trt_specular_project_scene.argtypes = [C.POINTER(L.Scene), C.POINTER(L.Screen), C.c_int, C.c_int, C.c_int, C.POINTER(Stats), C.POINTER(Log)]
    lib.trt_specular_project_scene.restype = None
    lib.trt_specular_shade_ray.argtypes = [C.POINTER(L.Scene), C.POINTER(L.Ray), C.c_int, C.c_void_p]
    lib.trt_specular_shade_ray.restype = C.c_int
    return lib


def render(scene_data, width, height, bounce_limit, rays_per_pixel, on, log=False):
    """(pixels [H, W, 3], (path rays, shadow rays), terms [n, TERM_DOUBLES] or None) of one frame of the restatement"""
    scene = scene_data.as_scene()
    screen, px = S.new_screen(width, height)
    st = Stats()
    if not (log and on):
        restatement().trt_specular_project_scene(C.byref(scene), C.byref(screen), bounce_limit, rays_per_pixel, int(on), C.byref(st), None)
        return px, (int(st.path_rays), int(st.shadow_rays)), None
    lights = len(scene_data.dir_lights) + len(scene_data.point_lights)
    cap = width * height * rays_per_pixel * bounce_limit * lights + 1
    terms = np.zeros((cap, TERM_DOUBLES))
    record = Log(terms.ctypes.data, cap, 0)
    restatement().trt_specular_project_scene(C.byref(scene), C.byref(screen), bounce_limit, rays_per_pixel, 1, C.byref(st), C.byref(record))
    assert record.count < cap, "the term log overflowed"
    return px, (int(st.path_rays), int(st.shadow_rays)), terms[: record.count].copy()


def shade_rays(scene_data, rays, on):
    """(what each ray met: 0 nothing, 1 a sphere, 2 the ground; the clamped colour of the point [n, 3]) as the probes report them"""
    scene = scene_data.as_scene()
    rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
    obj, lit = np.zeros(len(rays), dtype=np.int32), np.zeros((len(rays), 3))
    lib = restatement()
    for i in range(len(rays)):
        obj[i] = lib.trt_specular_shade_ray(C.byref(scene), C.byref(L.Ray.from_buffer(rays[i])), int(on), lit[i].ctypes.data)
    return obj, lit


def same(got, want, what):
    """frames that may hold values that are not finite: NaNs in the same places (x86-64 and the GPU make different NaNs), every other
    value -- the infinite ones too -- bit for bit"""
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaNs in other places", int((np.isnan(got) != np.isnan(want)).sum()))
    there = ~np.isnan(want)
    differ = T.bits(got)[there] != T.bits(want)[there]
    assert not differ.any(), (what, "values differ", int(differ.sum()), np.argwhere(T.bits(got) != T.bits(want))[:4].tolist())
