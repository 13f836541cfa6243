"""Candidate ENUMERATION, sphere by sphere and list entry by list entry (csrc/trt_rounds.hpp: trace(), point_light_search(); csrc/trt_tables.hip:
pack_cell()).  The tables and the FP32 sweep only propose spheres; that what they propose is conservative, and that the device builds the host
builders' masks and path cells, is proven elsewhere.  Here every ray is AIMED: its answer hangs on one known sphere at one known place -- sphere i
of a sweep of n (chunk and half-word boundaries, the padding of the last group, the second and third fixed-direction table), entry p of a list of K
(inline, pooled, either side of a pool word, 8- and 16-bit entries, the prefilter's compaction at its capacity and one over).

Two layers.  The CPU layer proves the aim: the oracle names the intended sphere, removing that sphere changes the oracle's lighting, and the cell
the host builders make for the ray has the intended encoding, length, position and number of filter survivors -- collected into a coverage table that
must equal the one written out below.  The GPU layer compares the production kernel's stages (trt_probe_rays_production) with the oracle bit for
bit on those rays, after requiring that the device's cells equal the classified ones.

Built as described in the issue except: the families of the spheres, their mirror images and the patches have the reduced set of directed cases
the issue names (one list per regime), at 8-bit entries, but no one-frame-per-regime renders of their own.  Whether the compaction is left at its capacity or one later (`nk > per_mask`) cannot be seen in an answer: either
way the same entries reach the exact test in the same order; only the count of exact tests differs, which the probe does not return."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import support as T
import test_raygrid as R
from support import bits
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S
from test_gpu_parity import _decode_cells

EYE_GRIDS = (4, 3)     # set_path_grids: a cell of the eye's table spans 22 degrees and more
LIGHT_GRIDS = (8, 2)   # set_light_grids, with set_light_slabs(1, 1): the coarsest tables the library builds


# ---- the host builds of the table headers ----

@functools.lru_cache(maxsize=None)
def raylib():
    lib = R.build_checker()
    lib.raygrid_cell_of.argtypes = [C.c_void_p, C.c_int]
    lib.raygrid_cell_of.restype = C.c_int
    lib.raygrid_member.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.raygrid_member.restype = C.c_int
    lib.raygrid_filter_survivors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.raygrid_filter_survivors.restype = C.c_int
    lib.raygrid_patch_of.argtypes = [C.c_int, C.c_void_p]
    lib.raygrid_patch_of.restype = C.c_int
    return lib


@functools.lru_cache(maxsize=None)
def lightlib():
    lib = T.lightgrid_checker()
    lib.lightgrid_host_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.lightgrid_host_table.restype = C.c_long
    lib.lightgrid_cell_of.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.lightgrid_cell_of.restype = C.c_long
    lib.lightgrid_pack.argtypes = [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long]
    lib.lightgrid_pack.restype = C.c_long
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def host_path_cells(scene, ge, gs, m=0):
    """the path rays' tables of the host reference builder, decoded: one tuple of sphere indices per cell"""
    n = len(scene.spheres)
    P = 6 * m * m if m else 1
    total = 2 * 6 * ge * ge + 2 * n * P * 6 * gs * gs
    cells, pool = np.zeros(total, dtype=np.uint64), np.zeros(2 * total + 16, dtype=np.uint64)
    sph, ground, eye = _f64(scene.spheres), _f64(scene.ground), _f64(scene.camera[9:12])
    used = raylib().raygrid_host_cells(sph.ctypes.data, n, ground.ctypes.data, eye.ctypes.data, ge, gs, m, cells.ctypes.data, pool.ctypes.data, len(pool))
    assert 0 <= used <= len(pool)
    return cells, _decode_cells(cells, pool, 16 if n > 256 else 8)


def host_light_lists(scene, kind, index, g, depth):
    """(raw cells, decoded lists) of one light's table: the host builder's masks packed with trt_list_pack"""
    sph = _f64(scene.spheres)
    n, words = len(sph), max(1, (len(sph) + 63) // 64)
    cells = depth * (g * g if kind == 0 else 6 * g * g)
    v = _f64(-scene.dir_lights[index, :3] if kind == 0 else scene.point_lights[index, :3])
    masks = np.zeros(cells * words, dtype=np.uint64)
    lightlib().lightgrid_host_table(sph.ctypes.data, n, kind, v.ctypes.data, g, depth, masks.ctypes.data)
    width = 16 if n > 256 else 8
    lists, pool = np.zeros(cells, dtype=np.uint64), np.zeros(cells * (words * 64 // (64 // width)) + 16, dtype=np.uint64)
    used = lightlib().lightgrid_pack(masks.ctypes.data, cells, words, width, lists.ctypes.data, pool.ctypes.data, len(pool))
    assert 0 <= used <= len(pool)
    return lists, _decode_cells(lists, pool, width)


def light_cell_of(scene, kind, index, g, depth, origin):
    sph, o = _f64(scene.spheres), _f64(origin)
    v = _f64(-scene.dir_lights[index, :3] if kind == 0 else scene.point_lights[index, :3])
    return lightlib().lightgrid_cell_of(sph.ctypes.data, len(sph), kind, v.ctypes.data, g, depth, o.ctypes.data)


def survivors(scene, ray, entries, fixed_dir=False):
    sph, ray, lst = _f64(scene.spheres), _f64(ray), np.ascontiguousarray(entries, dtype=np.int32)
    return raylib().raygrid_filter_survivors(sph.ctypes.data, len(sph), ray.ctypes.data, lst.ctypes.data, len(lst), int(fixed_dir))


def winner(scene, material):
    """the sphere a probe's material names (every sphere of a directed scene has a colour of its own)"""
    hit = np.nonzero((scene.spheres[:, 4:7] == material[:3]).all(axis=1))[0]
    assert len(hit) == 1, material
    return int(hit[0])


def same_probe(got, want, tag):
    """_same_probe of test_gpu_parity.py: bits of the doubles, `lit` only for hits"""
    obj, point, normal, material, lit = got
    assert np.array_equal(obj, want["obj"]), (tag, np.nonzero(obj != want["obj"])[0][:8])
    for name, a in (("point", point), ("normal", normal), ("material", material)):
        bad = np.nonzero((bits(a) != bits(want[name])).any(axis=1))[0]
        assert not len(bad), (tag, name, bad[:8], a[bad[:2]], want[name][bad[:2]])
    hit = obj != 0
    bad = np.nonzero(hit & (bits(lit) != bits(want["lit"])).any(axis=1))[0]
    assert not len(bad), (tag, "lit", bad[:8], lit[bad[:2]], want["lit"][bad[:2]])


# ---- (a), (b): the sweep ----

LIGHT_SETS = ((3, 2), (1, 0), (2, 1), (0, 1))  # directional, point lights of the (b) scenes: 1, 2 and 3 of the one kind, 0, 1 and 2 of the other; all for every n


@functools.lru_cache(maxsize=None)
def sweep_case(n):
    """[(tag, scene, rays, oracle's answers)] of n spheres: (a) with its twins, (b) per set of lights"""
    scene = T.sweep_scene(n, twins=T.sweep_twins(n))
    rays, _ = T.sweep_sphere_rays(scene)
    out = [("spheres", scene, rays, T.oracle_probe(scene, rays))]
    for nd, npt in LIGHT_SETS:
        scene = T.sweep_scene(n, nd, npt)
        rays = T.sweep_shadow_rays(scene)[0]
        out.append((f"shadows of {nd}+{npt} lights", scene, rays, T.oracle_probe(scene, rays)))
    return out


@pytest.mark.parametrize("n", T.SWEEP_COUNTS)
def test_every_sphere_of_a_sweep_has_a_ray_that_only_it_answers(n):
    """(a): the oracle names sphere i for ray i -- the lower index of a pair of twins --, for unit and non-unit directions; the misses miss"""
    _, scene, rays, want = sweep_case(n)[0]
    lower = {j: i for i, j in T.sweep_twins(n)}
    assert {(0, n - 1), (31, 32), (63, 64), (62, 65)} & set(T.sweep_twins(n)) == {t for t in ((0, n - 1), (31, 32), (63, 64), (62, 65)) if 2 <= n and t[1] < n}
    _, aimed = T.sweep_sphere_rays(scene)
    non_unit = np.abs((rays[:, 3:] ** 2).sum(axis=1) - 1.0) > 9.1e-13
    assert non_unit.sum() >= 3 and (aimed[non_unit] >= 0).any() and (aimed[non_unit] < 0).any()
    assert set(aimed[aimed >= 0]) == set(range(n))
    for k, i in enumerate(aimed):
        if i >= 0:
            assert want["obj"][k] == 1 and winner(scene, want["material"][k]) == lower.get(int(i), int(i)), (n, k, i)
        else:
            assert want["obj"][k] != 1, (n, k)
    assert (want["obj"][aimed < 0] == 0).any() and (want["obj"][aimed < 0] == 2).any()


@pytest.mark.parametrize("n", T.SWEEP_COUNTS)
def test_every_sphere_of_a_sweep_shadows_a_ground_point_of_every_light(n):
    """(b): every probe ray meets the ground; the oracle's lighting there CHANGES when the one sphere the point was made for is taken out of the
    scene, for every light; the points outside the lattice are lit as in a scene without spheres"""
    for (nd, npt), (_, scene, rays, want) in zip(LIGHT_SETS, sweep_case(n)[1:]):
        _, light, sphere = T.sweep_shadow_rays(scene)
        assert (want["obj"] == 2).all() and set(light[light >= 0]) == set(range(nd + npt))
        for i in range(n):
            mine = np.nonzero(sphere == i)[0]
            assert len(mine) == nd + npt
            bare = T.oracle_probe(T.without_sphere(scene, i), rays[mine])
            assert all(not np.array_equal(bare["lit"][a], want["lit"][k]) for a, k in enumerate(mine)), (n, nd, npt, i)
        free = sphere < 0
        assert free.sum() >= 4
        assert np.array_equal(bits(T.oracle_probe(scene.with_spheres(np.zeros((0, 9))), rays[free])["lit"]), bits(want["lit"][free]))


# ---- (c): lists of the eye's table ----

def regime(width, K, kept):
    per, inline = 64 // width, 56 // width
    if K <= inline:
        return "inline"
    if K <= 12:
        return "pooled"
    return "prefiltered, %s" % ("one survivor" if kept == 1 else "at capacity" if kept == per else "one over" if kept == per + 1 else "all survive" if kept == K else kept)


def lane_of(K, s, p):
    return (7 * K + 3 * s + p) % 64


@functools.lru_cache(maxsize=None)
def eye_case(K, s, p, wide, twin=None):
    scene, rays, index = T.eye_list_scene(K, s, p, wide, twin)
    probe = T.wave_layouts(rays, lane_of(K, s, p))
    return scene, rays, index, probe, T.oracle_probe(scene, probe)


def classify_eye_case(K, s, p, wide, twin=None):
    """(encoding, width, length, position of the winner, filter survivors) of the cell the directed ray reads in the host builder's table, after the
    conditions: the ray is a member of the eye's family, no cell it or its neighbours read lacks a list, the neighbours' cells are what
    the wave layouts need"""
    scene, rays, index, _, _ = eye_case(K, s, p, wide, twin)
    raw, lists = host_path_cells(scene, *EYE_GRIDS)
    sph, ground, eye = _f64(scene.spheres), _f64(scene.ground), _f64(scene.camera[9:12])
    seen = {}
    for name, ray in rays.items():
        ray = _f64(ray)
        assert raylib().raygrid_member(sph.ctypes.data, len(sph), ground.ctypes.data, eye.ctypes.data, 0, 0, ray.ctypes.data) == 1, name
        cell = raylib().raygrid_cell_of(ray[3:].ctypes.data, EYE_GRIDS[0])  # the eye's table comes first
        assert lists[cell] is not None, (name, "a cell without a list")
        seen[name] = (int(raw[cell]) >> 56, lists[cell])
    assert seen["main"][1] == tuple(index), (seen["main"][1], index)
    assert len(seen["short"][1]) == 1 and len(seen["over"][1]) == T.OVER_COUNT
    assert survivors(scene, rays["over"], seen["over"][1]) == T.OVER_COUNT > 8  # the neighbours' `over` is raised at either width
    want = T.oracle_probe(scene, rays["main"])
    assert want["obj"][0] == 1
    ctl, entries = seen["main"]
    width = 16 if len(sph) > 256 else 8
    assert all(e > 255 for e in entries[1:]) and entries[0] < 256 if wide else max(entries) < 256
    return ("pooled" if ctl & 0x80 else "inline", width, len(entries), entries.index(winner(scene, want["material"][0])), survivors(scene, rays["main"], entries))


# The coverage the builders must reach, written out: per entry width, every regime with the list lengths and the winner's positions it is met at.
COVERAGE = {
    8: {"inline": {(1, 0), (7, 0), (7, 6)},
        "pooled": {(8, 0), (8, 7), (9, 0), (9, 7), (9, 8), (12, 0), (12, 7), (12, 8), (12, 11)},
        "prefiltered, one survivor": {(K, p) for K in (13, 16, 17, 24, 25) for p in (0, 7, 8, K - 1)},
        "prefiltered, at capacity": {(K, p) for K in (13, 16, 17, 24, 25) for p in (0, 7, 8, K - 1)},
        "prefiltered, one over": {(K, p) for K in (13, 16, 17, 24, 25) for p in (0, 7, 8, K - 1)},
        "prefiltered, all survive": {(K, p) for K in (13, 16, 17, 24, 25) for p in (0, 7, 8, K - 1)}},
    16: {"inline": {(1, 0), (3, 0), (3, 2)},
         "pooled": {(4, 0), (4, 3), (5, 0), (5, 3), (5, 4), (8, 0), (8, 3), (8, 4), (8, 7), (9, 0), (9, 3), (9, 4), (9, 8), (12, 0), (12, 3), (12, 4), (12, 11)},
         "prefiltered, one survivor": {(K, p) for K in (13, 16, 17) for p in (0, 3, 4, K - 1)},
         "prefiltered, at capacity": {(K, p) for K in (13, 16, 17) for p in (0, 3, 4, K - 1)},
         "prefiltered, one over": {(K, p) for K in (13, 16, 17) for p in (0, 3, 4, K - 1)},
         "prefiltered, all survive": {(K, p) for K in (13, 16, 17) for p in (0, 3, 4, K - 1)}},
}
TWINS = {8: (16, 1, 7, False, (7, 8)), 16: (8, 1, 3, True, (3, 4))}  # two identical spheres either side of a pool-word boundary: the first must win


@pytest.mark.parametrize("wide", [False, True], ids=["8-bit entries", "16-bit entries"])
def test_directed_eye_lists_reach_the_cells_they_name(wide):
    """(c), the eye's family: every case's cell in the HOST builder's table has the encoding, the length, the winner's position and the number of
    filter survivors the case was built for, and together the cases cover the table written out above"""
    width = 16 if wide else 8
    found = {}
    for K, s, p in T.list_cases(wide):
        encoding, got_width, length, position, kept = classify_eye_case(K, s, p, wide)
        assert (got_width, length, position, kept) == (width, K, p, s), (K, s, p)
        assert encoding == ("inline" if K <= 56 // width else "pooled"), (K, encoding)
        found.setdefault(regime(width, K, kept), set()).add((length, position))
    assert found == COVERAGE[width], {k: found.get(k, set()) ^ COVERAGE[width].get(k, set()) for k in set(found) | set(COVERAGE[width])}
    encoding, got_width, length, position, kept = classify_eye_case(*TWINS[width])
    assert (encoding, got_width, length, position, kept) == ("pooled", width, TWINS[width][0], TWINS[width][2], 2)


# ---- (c), reduced: the families of a sphere, of its mirror image, and their patches ----

FAMILY_KINDS = [(kind, m) for kind in ("sphere", "mirror") for m in (0, 1, 2)]  # m: set_path_patches -- 1, 6 and 24 families per sphere and kind


@functools.lru_cache(maxsize=None)
def family_case(kind, K, s, p):
    """the scene; the ray of every role; for every role the pair (parent, ray) family_codes wants -- the parent of a sphere's ray is a stand-in that
    is not probed --; two waves of probe rays as T.wave_layouts makes them, with the roles of their lanes; the oracle's answers"""
    scene, rays, starts, index, source = T.family_list_scene(kind, K, s, p)
    probe = T.wave_layouts(rays, lane_of(K, s, p))
    roles = ["short"] * 64 + ["over"] * 64
    roles[lane_of(K, s, p)] = roles[64 + lane_of(K, s, p)] = "main"
    return scene, rays, starts, index, source, probe, roles, T.oracle_probe(scene, probe)


def family_table(scene, kind, m, source, start):
    """index, in the library's order, of the table a ray is looked up in: it (or its parent) started at `start` on sphere `source`"""
    P = 6 * m * m if m else 1
    w = _f64(start - scene.spheres[source, :3])
    return 2 + (len(scene.spheres) * P if kind == "mirror" else 0) + source * P + raylib().raygrid_patch_of(m, w.ctypes.data)


def classify_family_case(kind, m, K, s, p):
    """(regime, length, position of the winner) of the cell the directed ray reads in the host builder's tables of a sphere's families, after the
    conditions: every ray is a member of the table it is looked up in -- not the eye's, table index > 1 --, no cell read lacks a list, the
    neighbours' cells are what the wave layouts need"""
    scene, rays, starts, index, source, _, _, _ = family_case(kind, K, s, p)
    raw, lists = host_path_cells(scene, *EYE_GRIDS, m)
    sph, ground, eye = _f64(scene.spheres), _f64(scene.ground), _f64(scene.camera[9:12])
    seen, tables = {}, set()
    for name, ray in rays.items():
        ray = _f64(ray)
        table = family_table(scene, kind, m, source, starts[name])
        tables.add(table)
        assert table > 1 and raylib().raygrid_member(sph.ctypes.data, len(sph), ground.ctypes.data, eye.ctypes.data, m, table, ray.ctypes.data) == 1, (name, table)
        assert raylib().raygrid_member(sph.ctypes.data, len(sph), ground.ctypes.data, eye.ctypes.data, m, 0, ray.ctypes.data) == 0, name
        cell = 2 * 6 * EYE_GRIDS[0] ** 2 + (table - 2) * 6 * EYE_GRIDS[1] ** 2 + raylib().raygrid_cell_of(ray[3:].ctypes.data, EYE_GRIDS[1])
        assert lists[cell] is not None, (name, "a cell without a list")
        seen[name] = (int(raw[cell]) >> 56, lists[cell])
    assert len(tables) == (3 if m else 1)  # with patches every role starts on a patch of its own
    # a sphere sits in every cell of its own families: the source, of the highest index, is the last entry of its rays' lists
    own = (source,) if kind == "sphere" else ()
    assert seen["main"][1] == tuple(index) + own, (seen["main"][1], index)
    assert seen["short"][1][1:] == own and len(seen["over"][1]) == T.OVER_COUNT + len(own)
    assert survivors(scene, rays["over"], seen["over"][1]) >= T.OVER_COUNT > 8
    want = T.oracle_probe(scene, rays["main"])
    assert want["obj"][0] == 1
    ctl, entries = seen["main"]
    kept = survivors(scene, rays["main"], entries)
    assert s <= kept <= s + len(own)
    regime = "inline" if not ctl & 0x80 else "pooled" if len(entries) <= 12 else "prefiltered, compacted" if kept <= 8 else "prefiltered, overflowing"
    assert (regime == "inline") == (len(entries) <= 7)
    return regime, len(entries), entries.index(winner(scene, want["material"][0]))


FAMILY_COVERAGE = {(kind, m): {("inline", 5 + own, 4), ("pooled", 9 + own, 8), ("prefiltered, compacted", 16 + own, 7), ("prefiltered, overflowing", 16 + own, 8)}
                   for kind, own in (("sphere", 1), ("mirror", 0)) for m in (0, 1, 2)}


def test_directed_lists_of_a_spheres_families_reach_the_cells_they_name():
    """(c), reduced: one list per regime in the table of a sphere's family (code 2 + i), of its mirror image, and of their patches at
    set_path_patches(1) and (2) -- tables of index > 1, whose offset, membership test and (with patches) choice by the ray's origin the eye's cases
    do not meet"""
    found = {}
    for kind, m in FAMILY_KINDS:
        for K, s, p in T.FAMILY_CASES:
            found.setdefault((kind, m), set()).add(classify_family_case(kind, m, K, s, p))
    assert found == FAMILY_COVERAGE, {k: found[k] ^ FAMILY_COVERAGE[k] for k in found}


# ---- (d): lists of the light tables ----

def light_cases():
    """[(kind, K, p, wide, unsure, total spheres)]: K either side of inline / pooled / prefiltered, the blocker first, last and either side of a
    pool-word boundary; point lights also with a lone blocker about as far as the light; 16-bit entries once in a scene of more than 1024 spheres"""
    out = []
    for kind in (0, 1):
        for wide in (False, True):
            per = 4 if wide else 8
            for K in ((3, 9, 13) if wide else (7, 9, 17)):
                for p in sorted({0, K - 1, per - 1, per} & set(range(K))):
                    out.append((kind, K, p, wide, False, None))
            out.append((kind, 9, 4 if wide else 8, wide, False, 1100) if wide else (kind, 1, 0, wide, False, None))
        out += [(1, 9, 0, False, True, None), (1, 9, 0, True, True, None)]
    return out


def light_lanes(K, p):
    """where a (d) case sits in its two waves: (the directed point among empty cells, a neighbour there, the point among long lists, a neighbour there)"""
    lane = (5 * K + p) % 64
    return lane, (lane + 1) % 64, 64 + lane, 64 + (lane + 1) % 64


@functools.lru_cache(maxsize=None)
def light_case(kind, K, p, wide, unsure, total):
    """two waves, as T.wave_layouts makes them for the eye: the directed ground point among points whose cell is empty, then among points whose cell
    lists OVER_COUNT spheres that all pass the prefilter"""
    scene, rays, index = T.light_list_scene(kind, K, p, wide, unsure, total)
    probe = np.concatenate([np.tile(rays["other"], (64, 1)), np.tile(rays["over"], (64, 1))])
    probe[light_lanes(K, p)[0]] = probe[light_lanes(K, p)[2]] = rays["main"]
    return scene, rays, index, probe, T.oracle_probe(scene, probe)


def classify_light_case(kind, K, p, wide, unsure, total):
    scene, rays, index, probe, want = light_case(kind, K, p, wide, unsure, total)
    assert (want["obj"] == 2).all()
    lane, beside, lane2, beside2 = light_lanes(K, p)
    g = LIGHT_GRIDS[kind]
    raw, lists = host_light_lists(scene, kind, 0, g, 1)
    assert None not in lists
    point = want["point"][lane]  # the nudged ground point the shadow ray starts from
    cell, other = light_cell_of(scene, kind, 0, g, 1, point), light_cell_of(scene, kind, 0, g, 1, want["point"][beside])
    assert cell >= 0 and other >= 0 and cell != other
    entries = lists[cell]
    n = len(scene.spheres)
    blocker = n - 1 if unsure else index[p]
    assert entries == tuple(index) + ((n - 1,) if unsure else ()), (entries, index)
    assert len(lists[other]) <= (1 if unsure else 0)
    # the neighbours of the second wave: a long list of its own, every entry of which the prefilter keeps -- more than the compaction holds at
    # either width --, which darken the point
    assert np.array_equal(want["point"][lane2], point) and np.array_equal(want["lit"][lane2], want["lit"][lane])
    at = want["point"][beside2]
    over = lists[light_cell_of(scene, kind, 0, g, 1, at)]
    assert len(over) == T.OVER_COUNT + (1 if unsure else 0) > 12 and not set(over[:T.OVER_COUNT]) & set(index)
    to = T._unit(-scene.dir_lights[0, :3]) if kind == 0 else T._unit(scene.point_lights[0, :3] - at)
    assert survivors(scene, np.concatenate([at, to]), over[:T.OVER_COUNT], fixed_dir=kind == 0) == T.OVER_COUNT > 8
    bare = T.oracle_probe(scene.with_spheres(np.delete(scene.spheres, list(over[:T.OVER_COUNT]), axis=0)), rays["over"])
    assert unsure or not np.array_equal(bare["lit"][0], want["lit"][beside2])  # unsure: the sphere at the light darkens every point
    # the aim: without the blocker the oracle's lighting of the point changes; without any OTHER sphere of the cell it does not
    bare = T.oracle_probe(T.without_sphere(scene, blocker), rays["main"])
    assert not np.array_equal(bare["lit"][0], want["lit"][lane])
    for e in entries:
        if e != blocker:
            assert np.array_equal(T.oracle_probe(T.without_sphere(scene, e), rays["main"])["lit"][0], want["lit"][lane]), e
    to_light = T._unit(-scene.dir_lights[0, :3]) if kind == 0 else None
    kept = survivors(scene, np.concatenate([point, to_light]), entries, fixed_dir=True) if kind == 0 else None
    return ("pooled" if int(raw[cell]) >> 56 & 0x80 else "inline", 16 if n > 256 else 8, len(entries), entries.index(blocker), kept)


LIGHT_COVERAGE = {  # (kind, width): {(encoding, length, position of the blocker)}
    (0, 8): {("inline", 1, 0), ("inline", 7, 0), ("inline", 7, 6), ("pooled", 9, 0), ("pooled", 9, 7), ("pooled", 9, 8), ("pooled", 17, 0), ("pooled", 17, 7), ("pooled", 17, 8), ("pooled", 17, 16)},
    (0, 16): {("inline", 3, 0), ("inline", 3, 2), ("pooled", 9, 0), ("pooled", 9, 3), ("pooled", 9, 4), ("pooled", 9, 8), ("pooled", 13, 0), ("pooled", 13, 3), ("pooled", 13, 4), ("pooled", 13, 12)},
    (1, 8): {("inline", 1, 0), ("inline", 7, 0), ("inline", 7, 6), ("pooled", 9, 0), ("pooled", 9, 7), ("pooled", 9, 8), ("pooled", 17, 0), ("pooled", 17, 7), ("pooled", 17, 8), ("pooled", 17, 16),
             ("pooled", 10, 9)},
    (1, 16): {("inline", 3, 0), ("inline", 3, 2), ("pooled", 9, 0), ("pooled", 9, 3), ("pooled", 9, 4), ("pooled", 9, 8), ("pooled", 13, 0), ("pooled", 13, 3), ("pooled", 13, 4), ("pooled", 13, 12),
              ("pooled", 10, 9)},
}


def test_directed_light_lists_reach_the_cells_they_name():
    """(d): the cell a ground point's shadow ray reads in the HOST builder's table, packed as the library packs it, lists exactly the cluster; only
    the blocker at the intended position changes the oracle's lighting; the prefilter of a directional light's long list keeps that one sphere"""
    found = {}
    for case in light_cases():
        kind, K, p, wide, unsure, total = case
        encoding, width, length, position, kept = classify_light_case(*case)
        assert width == (16 if wide else 8) and (length, position) == ((K + 1, K) if unsure else (K, p)), case
        if kind == 0 and length > 12:
            assert kept == 1, case
        found.setdefault((kind, width), set()).add((encoding, length, position))
    assert found == LIGHT_COVERAGE, {k: found.get(k, set()) ^ LIGHT_COVERAGE.get(k, set()) for k in set(found) | set(LIGHT_COVERAGE)}


def test_the_lone_blocker_at_the_lights_distance_leaves_the_any_hit_search_unsure():
    """the `unsure` cases of (d): point_light_search, restated on the host (lightgrid_check.c), cannot decide the directed ray"""
    import test_lightgrid as LG
    lib = lightlib()
    lib.pointgrid_anyhit_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(LG.AnyHitStats)]
    lib.pointgrid_anyhit_check.restype = None
    for wide in (False, True):
        scene, rays, index, probe, want = light_case(1, 9, 0, wide, True, None)
        light = scene.point_lights[0, :3]
        point = want["point"][light_lanes(9, 0)[0]]  # the main ray's ground point
        st = LG.run_anyhit(lib, scene.spheres, scene.ground, light, np.concatenate([point, T._unit(light - point)]), LIGHT_GRIDS[1], 1)
        assert (st.rays, st.far, st.unsure, st.lit, st.dark) == (1, 0, 1, 0, 0), (st.rays, st.far, st.unsure, st.lit, st.dark)


def test_checker_helpers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the helpers this file and test_device_lookups.py add to raygrid_check.c, lean_lists_check.c and lightgrid_check.c (cell look-ups, membership, prefilter,
    packing; the host's look-up of many rays and the checks on a place the caller names), with the host builders
    they rest on, in a program of their own (tests/candidate_helpers_main.c) compiled with -fsanitize=address,undefined: a directed scene at
    either entry width must give the directed figures, and no report"""
    exe, inc = str(tmp_path / "candidate_helpers"), os.path.join(T.ROOT, "terminalraytracer_amd", "csrc")
    src = [os.path.join(T.ROOT, "tests", f) for f in ("candidate_helpers_main.c", "lean_lists_check.c", "lightgrid_check.c")]  # lean_lists_check.c includes raygrid_check.c
    subprocess.check_call(["gcc", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + inc, "-o", exe] + src + ["-lm"])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.endswith("ok\n") and not run.stderr, run.stdout[-2000:] + run.stderr[-3000:]


# ---- the GPU layer ----

@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.set_path_grids_min_spheres(0)
    yield c
    c.close()


def defaults(ctx):
    ctx.enable_counters(False)
    ctx.set_path_patches(-1)
    ctx.set_path_grids(64, 32)
    ctx.set_light_slabs(16, 16)
    ctx.set_light_grids(128, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", T.SWEEP_COUNTS)
def test_the_sweep_proposes_every_sphere_and_every_lights_blockers(ctx, n):
    """(a) and (b) through the production stages: every table off (path and shadow rays sweep; the second and third directional light read their own
    fixed-direction table), then the default tables (the shadow rays read the lights' lists; the path rays, given no family or the eye's, of which
    they are no members, still sweep: the path tables' lists are met by the (c) cases), and (a) through the reference-order kernel's probe"""
    try:
        for path_grids, light_grids in (((0, 0), (0, 0)), ((64, 32), (128, 64))):
            ctx.set_path_grids(*path_grids)
            ctx.set_light_grids(*light_grids)
            for tag, scene, rays, want in sweep_case(n):
                ctx.set_scene(scene)
                same_probe(ctx.probe_rays_production(scene.camera, rays), want, (n, tag, path_grids, "no family"))
                if path_grids[0]:
                    same_probe(ctx.probe_rays_production(scene.camera, rays, np.zeros(len(rays), dtype=np.int32)), want, (n, tag, "not members of the eye's family"))
        tag, scene, rays, want = sweep_case(n)[0]
        ctx.set_scene(scene)
        same_probe(ctx.probe_rays(rays), want, (n, tag, "reference-order kernel"))
    finally:
        defaults(ctx)


def device_eye_lists(ctx, scene):
    info, cells, pool = ctx.read_path_tables(scene.camera)
    assert info["enabled"] == 1 and (info["eye_cells"], info["sphere_cells"]) == EYE_GRIDS
    return _decode_cells(cells[:2 * 6 * EYE_GRIDS[0] ** 2], pool, 16 if len(scene.spheres) > 256 else 8)


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["8-bit entries", "16-bit entries"])
def test_every_list_position_of_the_eyes_cells_is_enumerated(ctx, wide):
    """(c) through the production stages with the eye's family code: the device's cells of the eye's two tables equal the host builder's (the ones the
    CPU layer classified), then each directed ray twice -- among short-list lanes, and among lanes whose lists overflow the prefilter's compaction"""
    try:
        ctx.set_path_patches(0)
        ctx.set_path_grids(*EYE_GRIDS)
        for case in [c + (wide,) for c in T.list_cases(wide)] + [TWINS[16 if wide else 8]]:
            scene, rays, index, probe, want = eye_case(*case)
            ctx.set_scene(scene)
            got = device_eye_lists(ctx, scene)
            assert got == host_path_cells(scene, *EYE_GRIDS)[1][:len(got)], case
            codes = ctx.family_codes(np.zeros(len(probe), dtype=np.int32), probe, len(scene.spheres))
            same_probe(ctx.probe_rays_production(scene.camera, probe, codes), want, case)
    finally:
        defaults(ctx)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [0, 1, 2], ids=["one family per sphere", "6 patches", "24 patches"])
def test_list_positions_of_a_spheres_families_are_enumerated(ctx, m):
    """(c), reduced, through the production stages with the codes of ctx.family_codes: rays that start on a sphere (2 + i: the kernel picks the patch
    from the origin) and rays the ground reflected (the code carries the parent's patch), after ALL the device's path cells equalled the host
    builder's; each directed ray among short-list lanes and among lanes that overflow the compaction"""
    try:
        ctx.set_path_patches(m)
        ctx.set_path_grids(*EYE_GRIDS)
        for kind in ("sphere", "mirror"):
            for case in T.FAMILY_CASES:
                scene, rays, starts, index, source, probe, roles, want = family_case(kind, *case)
                n = len(scene.spheres)
                ctx.set_scene(scene)
                assert ctx.path_patches() == (m, max(1, 6 * m * m))
                info, cells, pool = ctx.read_path_tables(scene.camera)
                assert info["enabled"] == 1 and (info["eye_cells"], info["sphere_cells"]) == EYE_GRIDS
                assert _decode_cells(cells, pool, 8) == host_path_cells(scene, *EYE_GRIDS, m)[1], (kind, m, case)
                if kind == "sphere":
                    codes = ctx.family_codes(np.full(len(probe), 2 + source, dtype=np.int32), probe, n)
                else:  # a mirror ray's code needs its parent in front of it: the ray that left the source sphere where the role's rays do
                    chain = np.zeros((2 * len(probe), 6))
                    chain[0::2, :3], chain[1::2] = [starts[r] for r in roles], probe
                    codes = ctx.family_codes(np.tile(np.array([2 + source, 2 + n + source], dtype=np.int32), len(probe)), chain, n)[1::2]
                    assert (codes >= 2 + n).all() and len(set(codes.tolist())) == (3 if m else 1)
                same_probe(ctx.probe_rays_production(scene.camera, probe, codes), want, (kind, m, case))
    finally:
        defaults(ctx)


@pytest.mark.gpu
def test_every_list_position_of_the_lights_cells_is_enumerated(ctx):
    """(d) through the production stages at the coarsest light tables: trace<true> with a list and the fixed-direction prefilter for the directional
    light, point_light_search -- and, for the lone blocker at the light's distance, the closest-hit search over the same cell -- for the point light;
    each directed point twice: among points whose cell is empty, and among points whose long lists overflow the prefilter's compaction;
    the device's list cells (trt_read_light_lists) equal the host builder's masks packed with trt_list_pack"""
    try:
        ctx.set_light_slabs(1, 1)
        ctx.set_light_grids(*LIGHT_GRIDS)
        for case in light_cases():
            kind = case[0]
            scene, rays, index, probe, want = light_case(*case)
            ctx.set_scene(scene)
            info, cells, pool = ctx.read_light_lists(kind, 0)
            assert info["enabled"] == 1 and info["list_bits"] == (16 if len(scene.spheres) > 256 else 8)
            assert _decode_cells(cells, pool, info["list_bits"]) == host_light_lists(scene, kind, 0, LIGHT_GRIDS[kind], 1)[1], case
            same_probe(ctx.probe_rays_production(scene.camera, probe), want, case)
    finally:
        defaults(ctx)


def packed_list_scenes():
    base = S.synth_scene(40, T.sky("synth"), T.bench_camera(32, 18), seed=5)
    c, r = base.spheres[3, :3], base.spheres[3, 3]
    lights = np.array([list(c + [0.0, r * 0.999, 0.0]) + [0.2, 1.0, 0.3, 9.0], list(c + [r * (1 + 1e-9), 0.0, 0.0]) + [1.0, 0.3, 0.2, 9.0],
                       [0.3, 7.0, -2.0, 1.0, 1.0, 1.0, 50.0], [40.0, 3.0, 11.0, 1.0, 1.0, 1.0, 900.0]])
    dirs = np.array([[0.0, -1.0, 0.0, 0.5, 0.5, 0.5], [1.0, -1e-9, 0.0, 0.3, 0.2, 0.1], [-0.3, -0.8, 0.55, 0.2, 0.3, 0.4]])
    # the three of test_device_built_light_tables_equal_the_host_reference_builder, then 16-bit entries
    return [S.synth_scene(64, T.sky("synth"), T.bench_camera(32, 18)), S.synth_scene(256, T.sky("synth"), T.bench_camera(32, 18)),
            S.SceneData(base.spheres, base.ground, dirs, lights, base.camera, base.sky), S.synth_scene(300, T.sky("synth"), T.bench_camera(32, 18), seed=11)]


@pytest.mark.gpu
def test_packed_light_lists_equal_the_host_packing_of_the_host_masks(ctx):
    """What the kernels read of a light's table is not the masks but the list cells pack_lists_kernel makes of them: every cell that has a list on
    both sides must list the same spheres in ascending order, and at the library's resolutions no cell may lack a list"""
    try:
        for scene in packed_list_scenes():
            n = len(scene.spheres)
            for gd, gp, sd, sp in ((128, 64, 16, 16), (19, 5, 1, 1)):  # the library's resolutions; coarse tables, whose lists are long
                ctx.set_scene(scene)
                ctx.set_light_slabs(sd, sp)
                ctx.set_light_grids(gd, gp)
                for kind, count, g, depth in ((0, len(scene.dir_lights), gd, sd), (1, len(scene.point_lights), gp, sp)):
                    for i in range(count):
                        info, cells, pool = ctx.read_light_lists(kind, i)
                        assert info["cells"] == len(cells) == depth * (g * g if kind == 0 else 6 * g * g) and info["list_bits"] == (16 if n > 256 else 8)
                        got, want = _decode_cells(cells, pool, info["list_bits"]), host_light_lists(scene, kind, i, g, depth)[1]
                        assert all(e is None or (list(e) == sorted(set(e)) and all(0 <= k < n for k in e)) for e in got)
                        bad = [k for k, (a, b) in enumerate(zip(got, want)) if a != b and a is not None and b is not None]
                        assert not bad, (n, kind, i, g, len(bad), bad[:3], [got[k] for k in bad[:3]], [want[k] for k in bad[:3]])
                        assert None not in want
                        if gd == 128:
                            assert None not in got
    finally:
        defaults(ctx)


def looking_along(camera, direction):
    """the camera turned so that the middle of its screen lies along `direction` (rays leave through a screen at -distance along the basis' z)"""
    cam = camera.copy()
    z = -T._unit(direction)
    x = T._unit(np.cross([0.0, 1.0, 0.0], z))
    cam[0:3], cam[3:6], cam[6:9] = x, np.cross(z, x), z
    return cam


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True], ids=["8-bit entries", "16-bit entries"])
def test_frames_of_the_directed_scenes_equal_the_oracle(ctx, wide):
    """the render kernel's own rounds through the long cells: a 24 x 16 frame at 2 rays per pixel, from the eye the directed rays start from and looking
    into their cell, of a prefiltered (c) scene and of a (d) scene per kind of light; framebuffer and trace counts against the oracle"""
    try:
        ctx.enable_counters(True)
        scene = eye_case(17, 5 if wide else 9, 4 if wide else 8, wide)[0]
        scene = scene.with_camera(looking_along(scene.camera, T.EYE_MAIN))
        frames = [(scene, EYE_GRIDS, (128, 64), (16, 16))]
        for kind in (0, 1):
            scene, rays = light_case(kind, 13 if wide else 17, 4 if wide else 8, wide, False, None)[:2]
            cam = scene.camera.copy()
            cam[9:12] = rays["main"][:3] + np.array([3.0, 6.0, 3.0])
            frames.append((scene.with_camera(looking_along(cam, [-3.0, -6.0, -3.0])), (64, 32), LIGHT_GRIDS, (1, 1)))
        for scene, path_grids, light_grids, slabs in frames:
            ctx.set_path_patches(0)
            ctx.set_path_grids(*path_grids)
            ctx.set_light_slabs(*slabs)
            ctx.set_light_grids(*light_grids)
            want, st = T.oracle_render(scene, 24, 16, 4, 2)
            got = T.render(ctx, scene, 24, 16, 4, 2)
            assert np.array_equal(bits(got), bits(want)), (len(scene.spheres), path_grids, light_grids)
            assert ctx.read_counters() == (st.path_rays, st.shadow_rays)
            assert len(np.unique(want.reshape(-1, 3), axis=0)) > 8  # the camera sees more than sky
    finally:
        defaults(ctx)
