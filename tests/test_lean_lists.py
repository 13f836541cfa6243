"""LEAN TWINS of the spheres' own families (csrc/trt_raygrid.h): a path ray that starts on sphere i and leaves it outwards --
(o - c_i).d >= 0, the very dot product the exact test forms -- reads its cell's list WITHOUT entry i, because that test answers
"miss" for every b = 2 (o - c_i).d >= 0 (TRT.c:657-659).  Host layer: the header's own stripping function (the one the device
kernel calls) against "the full list minus the own sphere" on real tables and on lists at every boundary of the encoding; the
sign argument and the twins' conservativeness on every path ray of real frames; rays directed through the tangent plane."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import support as T
from terminalraytracer_amd import scenes as S
from test_filter import traced_rays
from test_raygrid import FRAMES, _odd_scenes


class Stats(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("cells", "stripped", "unchanged", "no_list", "now_inline", "still_pooled", "copies", "pool_words", "violations",
                                             "rays", "own_members", "lean_rays", "lean_hits_own", "negative_hits_own", "candidates_full",
                                             "candidates_lean", "wave_max_full", "wave_max_lean", "wave_groups")] + \
               [("first_violation", C.c_double * 8)]


def build_checker():
    so = T.checker_so("libleanlistscheck")
    src = os.path.join(T.ROOT, "tests", "lean_lists_check.c")
    inc = os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")
    newest = max(os.path.getmtime(p) for p in (src, os.path.join(T.ROOT, "tests", "raygrid_check.c"), os.path.join(inc, "trt_raygrid.h"),
                                               os.path.join(inc, "trt_lightgrid.h"), os.path.join(inc, "trt_filter.h")))
    if not os.path.exists(so) or os.path.getmtime(so) < newest:
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-fPIC", "-shared"] + T.CHECKER_FLAGS +
                              ["-I" + inc, "-o", so, src, "-lm"])
    lib = C.CDLL(so)
    lib.lean_derive.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p, C.POINTER(C.c_long), C.c_long, C.c_int, C.POINTER(Stats)]
    lib.lean_derive.restype = None
    lib.lean_compare.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(Stats)]
    lib.lean_compare.restype = None
    lib.lean_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_long, C.POINTER(Stats)]
    lib.lean_build.restype = C.c_void_p
    lib.lean_free.argtypes = [C.c_void_p]
    lib.lean_free.restype = None
    lib.lean_rays_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(Stats)]
    lib.lean_rays_check.restype = None
    lib.lean_stats_clear.argtypes = [C.POINTER(Stats)]
    lib.lean_stats_clear.restype = None
    lib.lean_cell_entries.argtypes = [C.c_ulonglong, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.lean_cell_entries.restype = C.c_int
    lib.lean_same_entries.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_int]
    lib.lean_same_entries.restype = C.c_long
    return lib


@pytest.fixture(scope="module")
def checker():
    return build_checker()


def entries(checker, cell, pool, bits):
    out = np.zeros(1100, dtype=np.int32)
    e = checker.lean_cell_entries(int(cell), pool.ctypes.data, bits, out.ctypes.data, out.size)
    return None if e < 0 else [int(x) for x in out[:e]]


def pack(lst, bits, pool):
    """a list cell as trt_list_pack writes it (trt_raygrid.h): inline up to 7 / 3 entries, else words appended to `pool`"""
    per, inline_max = 64 // bits, 56 // bits
    if len(lst) <= inline_max:
        cell = len(lst) << 56
        for k, i in enumerate(lst):
            cell |= i << (bits * k)
        return cell
    at = len(pool)
    for w in range(0, len(lst), per):
        pool.append(sum(i << (bits * k) for k, i in enumerate(lst[w:w + per])))
    return (0x80 << 56) | (len(lst) << 32) | at


def derive(checker, cells, pool, bits, room):
    """twins of hand-made cells: cell c is its own one-cell table of sphere c; `room` pool words are free behind the full lists"""
    full = np.array(cells, dtype=np.uint64)
    lean = np.zeros_like(full)
    words = np.array(pool + [0] * (room + 1), dtype=np.uint64)
    used = C.c_long(len(pool))
    st = Stats()
    checker.lean_derive(full.ctypes.data, lean.ctypes.data, full.size, 1, 1, words.ctypes.data, C.byref(used), len(pool) + room, bits, C.byref(st))
    return full, lean, words, used.value, st


@pytest.mark.parametrize("bits", [8, 16])
def test_stripping_at_every_boundary_of_the_encoding(checker, bits):
    """8 -> 7 entries (4 -> 3 with 16 bits): pooled becomes inline; 9 -> 8 and 17 -> 16: one pool word less; 13 -> 12: the
    prefilter's threshold; the own sphere first, in the middle, last, alone, absent; a cell without a list; an empty cell."""
    per, inline_max = 64 // bits, 56 // bits
    sizes = sorted({1, 2, inline_max, inline_max + 1, inline_max + 2, per, per + 1, 2 * per, 2 * per + 1, 12, 13, 14, 40})
    top = 255 if bits == 8 else 1023
    lists, pool, cells = [], [], []
    for size in sizes:
        for where in ("first", "middle", "last", "absent"):
            c = len(cells)  # the own sphere of this cell
            assert c < top - 64
            others_below = list(range(0, c))[-size:]            # ascending indices below c
            others_above = list(range(c + 1, top + 1))[:size]   # and above
            if where == "first":
                lst = [c] + others_above[:size - 1]
            elif where == "last":
                lst = (others_below[-(size - 1):] if size > 1 else []) + [c]
            elif where == "middle":
                lo = others_below[-((size - 1) // 2):] if (size - 1) // 2 else []
                lst = lo + [c] + others_above[:size - 1 - len(lo)]
            else:
                lst = others_above[:size]
            assert len(lst) == size and lst == sorted(set(lst))
            lists.append(lst)
            cells.append(pack(lst, bits, pool))
    lists.append(None), cells.append(0xFF << 56)  # no list
    lists.append([]), cells.append(0)             # an empty list
    full, lean, words, used, st = derive(checker, cells, pool, bits, room=len(pool))
    assert st.violations == 0, list(st.first_violation)
    for c, lst in enumerate(lists):
        want = None if lst is None else [i for i in lst if i != c]
        assert entries(checker, lean[c], words, bits) == want, (c, lst)
        assert entries(checker, full[c], words, bits) == lst  # the full lists' words are untouched
        if lst is None or c not in lst:
            assert lean[c] == full[c]
        elif len(want) <= inline_max:
            assert int(lean[c]) >> 56 == len(want)
        else:
            assert int(lean[c]) >> 56 == 0x80 and len(pool) <= (int(lean[c]) & 0xFFFFFFFF) and (int(lean[c]) & 0xFFFFFFFF) + -(-len(want) // per) <= used
    assert st.now_inline == 3 and st.still_pooled > 0 and st.unchanged == len(sizes) + 2  # first / middle / last of the list one over the inline size
    # a pool with no room: the twins that would still be long lists are copies of their full cells, the others are as before
    full0, lean0, words0, used0, st0 = derive(checker, cells, pool, bits, room=0)
    assert st0.violations == 0 and used0 == len(pool) and st0.copies == st.still_pooled
    for c, lst in enumerate(lists):
        want = None if lst is None else [i for i in lst if i != c]
        long_twin = want is not None and len(want) > inline_max and c in lst
        assert entries(checker, lean0[c], words0, bits) == (lst if long_twin else want)
    # room for some: whichever twin finds none is a copy, never a list that runs past the room
    full1, lean1, words1, used1, st1 = derive(checker, cells, pool, bits, room=5)
    assert st1.violations == 0 and used1 <= len(pool) + 5 and 0 < st1.copies < st.still_pooled


SMALL = [("5 spheres", lambda: S.synth_scene(5, T.sky("synth"), T.bench_camera(64, 36)), [(5, 3, 0), (8, 8, 0), (5, 4, 1), (5, 3, 2)]),
         ("40 spheres", lambda: S.synth_scene(40, T.sky("synth"), T.bench_camera(64, 36, 10.0), seed=5), [(7, 3, 0), (16, 8, 0), (7, 4, 1), (7, 3, 2)]),
         # more than 256 spheres: 16-bit entries, 3 inline, 4 per pool word
         ("300 spheres", lambda: S.synth_scene(300, T.sky("synth"), T.bench_camera(64, 36), seed=11), [(7, 3, 0), (8, 8, 0), (7, 2, 1)])]


def host_tables(checker, scene, g_eye, g_sph, m, pool_cap=-1):
    sph = np.ascontiguousarray(scene.spheres, dtype=np.float64)
    ground = np.ascontiguousarray(scene.ground, dtype=np.float64)
    eye = np.ascontiguousarray(scene.camera[9:12], dtype=np.float64)
    st = Stats()
    handle = checker.lean_build(sph.ctypes.data, sph.shape[0], ground.ctypes.data, eye.ctypes.data, g_eye, g_sph, m, pool_cap, C.byref(st))
    return handle, st, sph


@pytest.mark.parametrize("name,make,grids", SMALL, ids=[s[0] for s in SMALL])
def test_every_twin_cell_is_the_full_cell_minus_the_own_sphere(checker, name, make, grids):
    scene = make()
    n = len(scene.spheres)
    for g_eye, g_sph, m in grids:
        handle, st, _ = host_tables(checker, scene, g_eye, g_sph, m)
        checker.lean_free(handle)
        P = 6 * m * m if m else 1
        print(f"\n{name} g {g_sph} m {m}: cells {st.cells} stripped {st.stripped} unchanged {st.unchanged} pooled -> inline {st.now_inline} "
              f"still pooled {st.still_pooled} pool words {st.pool_words}")
        assert st.violations == 0, list(st.first_violation)
        assert st.cells == n * P * 6 * g_sph * g_sph
        # a sphere sits in every cell of its own families: every twin is shorter, but for the cells that lost their list to the host pool
        assert st.stripped + st.no_list == st.cells and st.unchanged == st.no_list and st.copies == 0 and st.stripped > 0
        # a pool without room for the twins: whatever stays a long list is a copy, and still nothing is wrong
        handle, capped, _ = host_tables(checker, scene, g_eye, g_sph, m, pool_cap=0)
        checker.lean_free(handle)
        assert capped.violations == 0 and capped.pool_words == 0 and capped.still_pooled == 0 and (capped.copies > 0) == (st.still_pooled > 0)
        if st.no_list == 0:  # (which cells lose their list to an exhausted host pool depends on the order its threads ask in)
            assert capped.copies == st.still_pooled


def check_rays(checker, scene, rays, kinds, g_eye, g_sph, m, own=None):
    handle, st, sph = host_tables(checker, scene, g_eye, g_sph, m)
    try:
        assert st.violations == 0, list(st.first_violation)
        checker.lean_stats_clear(C.byref(st))
        rays = np.ascontiguousarray(rays, dtype=np.float64)
        kinds = None if kinds is None else np.ascontiguousarray(kinds, dtype=np.uint8)
        own = None if own is None else np.ascontiguousarray(own, dtype=np.int32)
        checker.lean_rays_check(handle, sph.ctypes.data, sph.shape[0], rays.ctypes.data, None if kinds is None else kinds.ctypes.data,
                                None if own is None else own.ctypes.data, rays.shape[0], C.byref(st))
    finally:
        checker.lean_free(handle)
    return st


def describe(st):
    m, g = max(st.own_members, 1), max(st.wave_groups, 1)
    return (f"path rays {st.rays}, memberships of an own family {st.own_members}, of which outwards {st.lean_rays} "
            f"({100.0 * st.lean_rays / m:.1f} %), hit their own sphere: outwards {st.lean_hits_own}, inwards {st.negative_hits_own}; "
            f"candidates per membership {st.candidates_full / m:.3f} -> {st.candidates_lean / m:.3f}, longest of 64 "
            f"{st.wave_max_full / g:.2f} -> {st.wave_max_lean / g:.2f}")


@pytest.mark.parametrize("name,make,w,h,b", FRAMES, ids=[f[0] for f in FRAMES])
def test_outward_rays_miss_their_own_sphere_and_twins_hold_every_hit_on_real_frames(checker, name, make, w, h, b):
    """Every path ray the oracle traces, in every own family it is a member of (not only the one the kernel would choose): a dot
    >= 0 implies that the reference's test of the own sphere misses, and every exact hit is in the list the ray reads."""
    scene = make()
    rays, kinds = traced_rays(scene, w, h, b, 10)
    n = len(scene.spheres)
    for g_eye, g_sph, m in ((64, 16 if n > 64 else 32, 0), (9, 4, 1)):
        st = check_rays(checker, scene, rays, kinds, g_eye, g_sph, m)
        print(f"\n{name} g {g_sph} m {m}: {describe(st)}")
        assert st.rays == int((kinds == 0).sum()) and st.violations == 0, list(st.first_violation)
        assert st.lean_hits_own == 0 and st.lean_rays > 0 and st.candidates_lean == st.candidates_full - st.lean_rays


@pytest.mark.parametrize("name,scene", _odd_scenes(), ids=[s[0] for s in _odd_scenes()])
def test_outward_rays_and_twins_on_adversarial_scenes(checker, name, scene):
    with np.errstate(all="ignore"):
        rays, kinds = traced_rays(scene, 64, 36, 8, 10)
    for m in (0, 2):
        st = check_rays(checker, scene, rays, kinds, 32, 8, m)
        print(f"\n{name}, patches m {m}: {describe(st)}")
        assert st.violations == 0 and st.lean_hits_own == 0, list(st.first_violation)


def directed_rays(scene_spheres, which, rng):
    """Rays that start 1e-6 off the surface of sphere `which` (outside and inside) with directions swept through the tangent plane
    in steps of a few ulp, then in coarser steps up to straight in and straight out."""
    c, r = scene_spheres[which, :3], abs(scene_spheres[which, 3])
    tilt = np.concatenate([np.arange(-8, 9) * 2.0 ** -52, np.arange(-8, 9) * 2.0 ** -50, [s * 10.0 ** e for e in (-14, -12, -9, -6, -4, -2) for s in (-1, 1)],
                           [-0.5, 0.5, -1e6, 1e6]])
    rays = []
    for _ in range(24):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        t = np.cross(u, rng.normal(size=3))
        t /= np.linalg.norm(t)
        for off in (1e-6, -1e-6, 0.0, 3e-6):
            o = c + (r + off) * u
            for e in tilt:
                d = t + e * u
                rays.append(np.concatenate([o, d / np.linalg.norm(d)]))
    return np.array(rays)


def test_rays_directed_through_the_tangent_plane(checker):
    """Two spheres share a centre (only index i leaves the list of family i), one has a radius below 1e-4.  Rays aimed inwards from
    outside the surface do hit their own sphere: they have a negative dot and are answered from the full list, which holds it."""
    base = S.synth_scene(12, T.sky("synth"), T.bench_camera(64, 36))
    sph = base.spheres.copy()
    sph[1, :3] = sph[0, :3]
    sph[1, 3] = sph[0, 3] * 1.25  # the same centre, another radius
    sph[2, 3] = 5e-5
    sph[3, :3] = sph[4, :3] + [sph[4, 3] + sph[3, 3], 0.0, 0.0]  # touching
    scene = base.with_spheres(sph)
    rng = np.random.default_rng(7)
    rays, own = [], []
    for i in (0, 1, 2, 3, 4, 7):
        r = directed_rays(sph, i, rng)
        rays.append(r), own.append(np.full(len(r), i))
    rays, own = np.concatenate(rays), np.concatenate(own)
    for g_sph, m in ((16, 0), (4, 1), (4, 2)):
        st = check_rays(checker, scene, rays, None, 8, g_sph, m, own=own)
        print(f"\ng {g_sph} m {m}: {describe(st)}")
        assert st.violations == 0 and st.lean_hits_own == 0, list(st.first_violation)
        assert st.negative_hits_own > 100 and st.lean_rays > 1000 and st.own_members - st.lean_rays > 1000
