"""WHERE THE DEVICE LOOKS.  The candidate tables and the FP32 filter only propose spheres, and what they propose is conservative -- proven on the
host, for the cell the HOST headers look up (test_lightgrid, test_raygrid, test_filter, test_lean_lists), and the device builds the same tables
(test_gpu_parity).  This file holds the device's own look-ups against those proofs: the render kernels' path_cell / path_cell_patches, the shading
stage's look-up lines and the filter report where they looked (trt_probe_path_lookups, trt_probe_shadow_lookups, trt_selftest_filter), and

  A  what is made of IEEE operations alone agrees with the host bit for bit: the filter's fields and sign words, trt_dirgrid_cell's cell and far,
     the membership verdict of a path ray, the bounds of the point lights' any-hit search;
  B  where v_rcp_f32 or v_sqrt_f32 enters (the cube maps' cells, the patch choice, the point lights' cells and shells) the face is the host's and
     column, row and shell are the host's or a neighbour's, on random rays in at most 1e-4 of the look-ups;
  C  the host's conservativeness checks, given the DEVICE's place, find nothing, and the cell word the device read lists what the host's table
     lists at that place;
  D  a ray falls back exactly when it is no member of the table the device used or that cell has no list, the table is the one the family code
     names (the frame's eye slot, the patch, the mirror block, the lean twin exactly where the ray leaves its own sphere outwards), and the
     successor code is the host's.

Two layers, as in test_candidate_edges.py: the CPU layer proves that the inputs are aimed (bisected cell edges differ on the host, every
membership threshold has members and non-members, the host's own look-ups are conservative and not vacuous), the GPU layer asserts A to D.

As built: without patches the look-up does not rewrite the family code (path_stage forms the successor), so the successor is checked with patches
only.  The library builds no directional table of fewer than 8 cells per side: the coarsest light tables are 8 (directional) and 4 (point) cells.
NaN results (rays that are not `ok`, a culling table that overflowed) compare as NaN, not by payload: x86 and gfx950 give their default NaN different
sign bits.  At 1e+18 the filter's bounds of these scenes stay just inside FP32; a third scale, 1e+20, is where they overflow.  The shadow look-ups
of the scene of 300 spheres take 1e5 origins per light (the host's checks cost three exact tests per sphere and origin).

Found with it: trt_set_scene grew the scene's part of the pool of long lists on paper after its last build pass when the lean twins asked for more
words than the first pass could count (300 spheres with patches and twins); the eye slots' parts then lay behind the end of the pool, and a batch
of eight cameras faulted in the builder of the last slots' tables (fixed in csrc/trt_tables.hip: build_tables)."""
import ctypes as C
import functools

import numpy as np
import pytest

import support as T
import test_lean_lists as LL
import test_lightgrid as LG
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S

COUNTS = (3, 70, 300)                                  # the smallest scene | two mask words, 8-bit entries | 16-bit entries
PATH_GRIDS = {3: (64, 32), 70: (8, 4), 300: (8, 4)}    # set_path_grids: the default, then coarse tables whose lists are long
PATCHES = (0, 1, 2)
LIGHT_GRIDS = ((8, 4, 1), (32, 32, 5), (128, 128, 16)) # directional cells, point cells, slabs = shells
FRAMES = (0, 1, 7)                                     # of eight cameras whose eyes differ
SHIFT = 7                                              # TRT_PATCH_SHIFT
UNIT_TOL = 9.094947017729282e-13                       # 2^-40
CLASSES = ("random", "direction edges", "patch edges", "cube edges", "thresholds", "family kinds", "lean twin", "non-finite")
LIGHT_CLASSES = ("random", "cell edges", "cube edges", "thresholds", "non-finite")


class Judged(C.Structure):
    _fields_ = [(k, C.c_ulonglong) for k in ("rays", "judged", "no_place", "strangers", "no_list", "exact_hits", "candidates", "violations", "lean_reads",
                                             "lean_misses_own", "full_hits_own")] + [("first_violation", C.c_double * 8)]


_VP, _I, _SZ, _L = C.c_void_p, C.c_int, C.c_size_t, C.c_long


@functools.lru_cache(maxsize=None)
def pathlib():
    lib = LL.build_checker()
    for name, res, args in (("lookup_host_build", _VP, [_VP, _I, _VP, _VP, _I, _I, _I, _I]),
                            ("lookup_path_host", None, [_VP, _VP, _VP, _VP, _VP, _SZ, _VP, _VP]),
                            ("lookup_path_members", None, [_VP, _VP, _VP, _VP, _SZ, _VP]),
                            ("lookup_path_judge", None, [_VP, _VP, _VP, _VP, _VP, _VP, _SZ, C.POINTER(Judged)]),
                            ("lookup_path_same_entries", _L, [_VP, _VP, _VP, _VP, _VP, _VP, _L, _SZ]),
                            ("lookup_cubemap_cells", None, [_VP, _SZ, _I, _VP]),
                            ("lookup_family_record", _I, [_VP, _I, _I, _VP]),
                            ("lookup_along", None, [_VP, _VP, _VP, _SZ, _VP]),
                            ("lookup_host_info", None, [_VP, _VP])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


@functools.lru_cache(maxsize=None)
def lightlib():
    lib = T.lightgrid_checker()
    for name, res, args in (("light_host_build", _VP, [_VP, _I, _I, _VP, _I, _I]),
                            ("light_host_lookup", None, [_VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP]),
                            ("lightgrid_check_at", None, [_VP, _VP, _VP, _VP, _SZ, C.POINTER(LG.Stats)]),
                            ("pointgrid_anyhit_check_at", None, [_VP, _VP, _VP, _VP, _VP, _SZ, C.POINTER(LG.AnyHitStats)]),
                            ("light_host_same_entries", _L, [_VP, _VP, _VP, _VP, _L, _I, _SZ]),
                            ("light_host_range", None, [_VP, _VP]),
                            ("light_host_coords", None, [_VP, _VP, _SZ, _VP]),
                            ("filter_host_words", None, [_VP, _I, _VP, _SZ, _VP, _VP, _VP, _VP])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _unit(v):
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _rand_unit(rng, k):
    return _unit(rng.normal(size=(k, 3)))


def step_ulps(x, k):
    """x moved k representable doubles along the number line (k an integer array of x's shape; -0.0 and +0.0 are one place)"""
    i = _f64(x).view(np.int64)
    mag = i & np.int64(0x7FFFFFFFFFFFFFFF)
    o = np.where(i < 0, -mag, mag) + np.asarray(k, dtype=np.int64)
    return np.where(o < 0, (-o) | np.int64(-2 ** 63), o).view(np.float64)


# ---- scenes and cameras ----

@functools.lru_cache(maxsize=None)
def scene(n):
    """n synthetic spheres, two directional lights, two point lights, one of them close to sphere 0"""
    base = S.synth_scene(n, T.sky("synth"), T.bench_camera(32, 18), seed=40 + n)
    c, r = base.spheres[0, :3], base.spheres[0, 3]
    dirs = np.array([[-0.3, -1.0, -0.2, 0.3, 0.3, 0.3], [0.45, -0.8, 0.4, 0.2, 0.2, 0.2]])
    points = np.array([[4.0, 9.0, -3.0, 1.0, 1.0, 1.0, 60.0], list(c + np.array([1.3 * r, 0.4 * r, 0.0])) + [1.0, 0.3, 0.2, 2.0]])
    return S.SceneData(base.spheres, base.ground, dirs, points, base.camera, base.sky)


@functools.lru_cache(maxsize=None)
def cameras():
    """eight cameras whose eyes differ"""
    cams = np.tile(T.bench_camera(32, 18), (8, 1))
    cams[:, 9:12] += np.arange(8)[:, None] * np.array([0.7, 0.3, -0.5])
    return cams


def mirror_point(p, ground):
    nrm = ground[3:6]
    return p - 2.0 * (((p - ground[:3]) @ nrm) / (nrm @ nrm))[:, None] * nrm


# ---- the host's side of the path rays' look-ups ----

@functools.lru_cache(maxsize=None)
def path_host(n, m):
    """the host reference tables of scene(n) with patches m for the eight eyes, and their twins (tests/lean_lists_check.c)"""
    sc, eyes = scene(n), _f64(cameras()[:, 9:12])
    h = pathlib().lookup_host_build(_f64(sc.spheres).ctypes.data, n, _f64(sc.ground).ctypes.data, eyes.ctypes.data, 8, *PATH_GRIDS[n], m)
    assert h, "the host's twins failed their own check"
    info = (C.c_long * 4)()
    pathlib().lookup_host_info(h, info)
    assert info[1] == 0, "a cell of the host's tables found no room for its list"
    return h


def host_lookup(n, m, rays, codes, frames):
    """the host's own look-up: dict of region, table, cell, member, successor, patch, has_list, lean per ray, and the cell words"""
    rays, codes, frames = _f64(rays), _i32(codes), _i32(frames)
    out, words = np.zeros((len(rays), 8), dtype=np.int32), np.zeros(len(rays), dtype=np.uint64)
    pathlib().lookup_path_host(path_host(n, m), _f64(scene(n).spheres).ctypes.data, rays.ctypes.data, codes.ctypes.data, frames.ctypes.data, len(rays),
                               out.ctypes.data, words.ctypes.data)
    got = {k: out[:, j].copy() for j, k in enumerate(("region", "table", "cell", "member", "successor", "patch", "has_list", "lean"))}
    got["word"] = words
    return got


def members_of(n, m, rays, region, table):
    rays, region, table = _f64(rays), _i32(region), _i32(table)
    out = np.zeros(len(rays), dtype=np.int32)
    pathlib().lookup_path_members(path_host(n, m), rays.ctypes.data, region.ctypes.data, table.ctypes.data, len(rays), out.ctypes.data)
    return out


def judge(n, m, rays, region, table, cell):
    rays, region, table, cell = _f64(rays), _i32(region), _i32(table), _i32(cell)
    st = Judged()
    pathlib().lookup_path_judge(path_host(n, m), _f64(scene(n).spheres).ctypes.data, rays.ctypes.data, region.ctypes.data, table.ctypes.data, cell.ctypes.data,
                                len(rays), C.byref(st))
    return st


def cube_cells(w, g):
    w = _f64(w).reshape(-1, 3)
    out = np.zeros(len(w), dtype=np.int32)
    pathlib().lookup_cubemap_cells(w.ctypes.data, len(w), g, out.ctypes.data)
    return out


def family_record(n, m, region, table):
    out = np.zeros(6)
    assert pathlib().lookup_family_record(path_host(n, m), region, table, out.ctypes.data) == 1, (region, table)
    return out[:3].copy(), out[3], out[5]  # apex, r_chk, rg^2


def face_row_col(cell, g):
    cell = np.asarray(cell, dtype=np.int64)
    return cell // (g * g), (cell // g) % g, cell % g


# ---- inputs: bisection ----

def bisect(a, b, cell_of):
    """pairs a[k], b[k] whose host cells differ, halved until every component of a and b is the same or a neighbouring double: the pair straddles
    an edge of the look-up, wherever that edge is.  Returns (a, b)."""
    a, b = _f64(a).copy(), _f64(b).copy()
    ca = cell_of(a)
    assert (ca != cell_of(b)).all()
    for _ in range(80):
        mid = 0.5 * (a + b)
        done = ((mid == a) | (mid == b)).all(axis=1)
        if done.all():
            break
        left = cell_of(mid) == ca
        a = np.where((left & ~done)[:, None], mid, a)
        b = np.where((~left & ~done)[:, None], mid, b)
    assert done.all() and (cell_of(a) == ca).all() and (cell_of(b) != ca).all()
    return a, b


def bisect_directions(a, b, cell_of):
    """the same for UNIT vectors, which a path ray's direction must be: the pair is d(t) = unit(a + t (b - a)) at two neighbouring doubles t, found
    by halving [0, 1].  Returns [(k, d(t_lo moved k doubles down), d(t_hi moved k doubles up))] for the neighbours k."""
    point = lambda t: _unit(a + t[:, None] * (b - a))
    lo, hi = np.zeros(len(a)), np.ones(len(a))
    ca = cell_of(point(lo))
    assert (ca != cell_of(point(hi))).all()
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        done = (mid == lo) | (mid == hi)
        if done.all():
            break
        left = cell_of(point(mid)) == ca
        lo, hi = np.where(left & ~done, mid, lo), np.where(~left & ~done, mid, hi)
    assert done.all() and (cell_of(point(lo)) == ca).all() and (cell_of(point(hi)) != ca).all()
    return [(k, point(step_ulps(lo, np.full(len(lo), -k))), point(step_ulps(hi, np.full(len(hi), k)))) for k in NEIGHBOURS]


NEIGHBOURS = (0, 1, 2, 8)


def straddle(a, b):
    """the 0, +-1, +-2, +-8 neighbours of a bisected pair: [(k, a moved k doubles away from b, b moved k doubles away from a)]"""
    s = np.sign(b - a).astype(np.int64)
    return [(k, step_ulps(a, -k * s), step_ulps(b, k * s)) for k in NEIGHBOURS]


def differing_pairs(rng, count, make, cell_of):
    """`count` pairs (a, b) = make(rng, k) whose host cells differ"""
    got_a, got_b = np.zeros((0, 3)), np.zeros((0, 3))
    for _ in range(40):
        a, b = make(rng, 4 * count)
        keep = cell_of(a) != cell_of(b)
        got_a, got_b = np.concatenate([got_a, a[keep]]), np.concatenate([got_b, b[keep]])
        if len(got_a) >= count:
            return got_a[:count], got_b[:count]
    raise AssertionError("no pairs of inputs whose cells differ")


def special_vectors():
    """cube edges and corners: components of equal magnitude and a hair apart, axis directions, components that are 0, -0.0 or an FP32 denormal"""
    out = []
    h = np.sqrt(0.5)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for tiny in (0.0, -0.0, 1e-40, -1e-40):
                for perm in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
                    for y in (h, np.nextafter(h, 1.0), np.nextafter(h, 0.0), np.float64(np.float32(h)), np.float64(np.nextafter(np.float32(h), np.float32(1.0)))):
                        v = np.array([sx * h, sy * y, tiny])[list(perm)]
                        out.append(v)
            for sz in (1.0, -1.0):
                t = np.sqrt(1.0 / 3.0)
                out.append(np.array([sx * t, sy * t, sz * t]))
                out.append(np.array([sx * t, sy * np.nextafter(t, 1.0), sz * np.nextafter(t, 0.0)]))
    for axis in range(3):
        for s in (1.0, -1.0):
            for tiny in (0.0, -0.0, 1e-40):
                v = np.full(3, tiny)
                v[axis] = s
                out.append(v)
    return np.array(out)


# ---- inputs: path rays ----

def family_code(n, m, i, k, mirrored):
    if not mirrored:
        return 2 + i
    return 2 + n + (((i << SHIFT) | k) if m else i)


@functools.lru_cache(maxsize=None)
def path_inputs(n, m):
    """rays [N, 6], family codes, frames, class (index into CLASSES) and what the CPU layer needs to prove the aim"""
    rng = np.random.default_rng(1000 * n + m)
    sc = scene(n)
    sph, ground, eyes = sc.spheres, sc.ground, cameras()[:, 9:12]
    ge, gs = PATH_GRIDS[n]
    parts, aim = [], {"pairs": {}, "thresholds": {}}

    def add(cls, rays, codes, frames):
        rays = _f64(rays).reshape(-1, 6)
        parts.append((np.full(len(rays), CLASSES.index(cls), dtype=np.int32), rays, np.broadcast_to(_i32(codes), (len(rays),)).copy(),
                      np.broadcast_to(_i32(frames), (len(rays),)).copy()))
        return slice(sum(len(p[0]) for p in parts[:-1]), sum(len(p[0]) for p in parts))

    def aimed(o):
        """directions from the origins o: towards a point near some sphere, four in ten anywhere"""
        j = rng.integers(n, size=len(o))
        d = _unit(sph[j, :3] + sph[j, 3:4] * rng.uniform(-1.3, 1.3, (len(o), 3)) - o)
        anywhere = rng.random(len(o)) < 0.4
        d[anywhere] = _rand_unit(rng, int(anywhere.sum()))
        return d

    def patch_of(w):
        return cube_cells(w, m) if m else np.zeros(len(w), dtype=np.int32)

    def on_sphere(k):
        i = rng.integers(n, size=k)
        u = _rand_unit(rng, k)
        return i, sph[i, :3] + (sph[i, 3:4] * (1.0 + 1e-6)) * u

    def eye_rays(k):
        f = rng.choice(FRAMES, size=k)
        return np.concatenate([eyes[f], aimed(eyes[f])], axis=1), f

    def mirror_eye_rays(k):
        f = rng.choice(FRAMES, size=k)
        apex = np.array([family_record(n, m, 0, 2 * b + 1)[0] for b in range(8)])[f]
        d = aimed(apex)
        return np.concatenate([apex + d * rng.uniform(0.3, 6.0, (k, 1)), d], axis=1), f

    def sphere_rays(k):
        i, o = on_sphere(k)
        return i, np.concatenate([o, aimed(o)], axis=1)

    def mirror_sphere_rays(k):
        i, o = on_sphere(k)
        kk = patch_of(o - sph[i, :3])
        o = mirror_point(o, ground)
        return i, kk, np.concatenate([o, aimed(o)], axis=1)

    # random rays of every family kind
    q = 30000
    rays, f = eye_rays(q)
    add("random", rays, 0, f)
    rays, f = mirror_eye_rays(q)
    add("random", rays, 1, f)
    i, rays = sphere_rays(q)
    add("random", rays, 2 + i, rng.choice(FRAMES, size=q))
    i, kk, rays = mirror_sphere_rays(q)
    add("random", rays, [family_code(n, m, a, b, True) for a, b in zip(i, kk)], rng.choice(FRAMES, size=q))
    aim["patches seen"] = (set(patch_of(parts[2][1][:, :3] - sph[parts[2][2] - 2, :3]).tolist()), set(kk.tolist()))

    # directions across cell edges of the eye's and the spheres' cube maps
    def near_directions(g):
        def make(rng, k):
            a = _rand_unit(rng, k)
            return a, _unit(a + (2.0 / g) * rng.normal(size=(k, 3)))
        return make

    for name, g in (("eye", ge), ("sphere", gs)):
        cell_of = functools.partial(cube_cells, g=g)
        for k, lo, hi in bisect_directions(*differing_pairs(rng, 1200, near_directions(g), cell_of), cell_of):
            aim["pairs"][("direction", name, k)] = (cell_of(lo), cell_of(hi))
            for d in (lo, hi):
                if name == "eye":
                    f = rng.choice(FRAMES, size=len(d))
                    add("direction edges", np.concatenate([eyes[f], d], axis=1), 0, f)
                else:  # from the surface of a sphere, straight out (the twin) or straight in (the full table)
                    i = rng.integers(n, size=len(d))
                    out = rng.random(len(d)) < 0.5
                    o = sph[i, :3] + (sph[i, 3:4] * (1.0 + 1e-6)) * np.where(out[:, None], d, -d)
                    add("direction edges", np.concatenate([o, d], axis=1), 2 + i, 0)

    # origins across patch edges
    if m:
        i = rng.integers(n, size=1)[0]
        c, r = sph[i, :3], sph[i, 3]
        cell_of = lambda o: cube_cells(o - c, m)

        def make(rng, k):
            u = _rand_unit(rng, k)
            return c + r * u, c + r * _unit(u + 0.8 * rng.normal(size=(k, 3)))
        a, b = bisect(*differing_pairs(rng, 1200, make, cell_of), cell_of)
        for k, lo, hi in straddle(a, b):
            aim["pairs"][("patch", i, k)] = (cell_of(lo), cell_of(hi))
            for o in (lo, hi):
                add("patch edges", np.concatenate([o, _unit(_unit(o - c) + 0.5 * rng.normal(size=o.shape))], axis=1), 2 + i, 0)

    # cube edges and corners, as directions and as origins on a sphere; an origin at a sphere's centre
    v = special_vectors()
    vu = _unit(v)
    add("cube edges", np.concatenate([np.tile(eyes[0], (len(v), 1)), vu], axis=1), 0, 0)
    for i in sorted({0, n // 2, n - 1}):
        c, r = sph[i, :3], sph[i, 3]
        add("cube edges", np.concatenate([c + (r * (1.0 + 1e-6)) * v, vu], axis=1), 2 + i, 0)
        add("cube edges", np.concatenate([c + r * v, _unit(vu + 0.3 * rng.normal(size=v.shape))], axis=1), 2 + i, 0)
        add("cube edges", np.concatenate([np.tile(c, (len(v), 1)), vu], axis=1), 2 + i, 0)

    # membership thresholds, either side: one family of every kind
    eps = np.array([s * e for e in (2.0 ** -52, 2.0 ** -51, 2.0 ** -49, 1e-12, 1e-9) for s in (1.0, -1.0)])
    kinds = [("eye", 0, 2 * 1 + 0, 0, 1, None), ("mirror eye", 0, 2 * 7 + 1, 1, 7, None)]
    P = 6 * m * m if m else 1
    for i in sorted({0, n - 1}):
        for k in sorted({0, P // 2, P - 1}):
            kinds.append(("sphere", 1, i * P + k, family_code(n, m, i, k, False), 0, (i, k)))
            kinds.append(("mirror sphere", 1, (n + i) * P + k, family_code(n, m, i, k, True), 0, None))
    for name, region, table, code, frame, own in kinds:
        apex, r_chk, rg2 = family_record(n, m, region, table)
        count = 40
        e = np.repeat(eps, count)[:, None]
        # a sphere's own family is chosen by the ORIGIN's patch: the rays keep their origin over the middle of the patch, along the apex's offset
        prefer = None
        if own is not None and m:
            prefer = _unit(apex - sph[own[0], :3])
        qv = np.tile(prefer, (len(e), 1)) if prefer is not None else _rand_unit(rng, len(e))
        across = _unit(np.cross(qv, rng.normal(size=qv.shape)))
        t = rng.uniform(0.5, 2.0, (len(e), 1)) if prefer is None else 0.0
        made = {"near line": (apex + qv * (r_chk * (1.0 + e)) + across * t, across),
                "ahead": (apex + qv * (r_chk * (1.0 + e)), -qv),
                "in range": (apex + qv * (np.sqrt(rg2) * (1.0 + e)), qv)}
        s = np.repeat(np.array([a * 2.0 ** -41 * (1.0 + b) for a in (1.0, -1.0) for b in (0.0, 2.0 ** -10, -2.0 ** -10, 1e-3, -1e-3)]), count)[:, None]
        made["unit direction"] = (apex + qv * (0.5 * r_chk) + across * t, across * (1.0 + s))
        for what, (o, d) in made.items():
            aim["thresholds"].setdefault(what, []).append((add("thresholds", np.concatenate([o, d], axis=1), code, frame), region, table))

    # every family kind: no family, another sphere's code, the other eye family, codes the kernel cannot decode, another patch, another frame
    i, rays = sphere_rays(3000)
    add("family kinds", rays, 2 + (i + 1) % n, 0)
    add("family kinds", rays[:1000], -1, 0)
    add("family kinds", rays[:300], [2 + 2 * n + (n << SHIFT if m else 0), 10 ** 6, -7] * 100, 0)
    rays, f = eye_rays(3000)
    add("family kinds", rays[:1000], 1, f[:1000])
    add("family kinds", rays, 0, np.array(FRAMES)[(np.searchsorted(FRAMES, f) + 1) % 3])  # a ray of frame b given to frame b'
    rays, f = mirror_eye_rays(1000)
    add("family kinds", rays, 0, f)
    i, kk, rays = mirror_sphere_rays(2000)
    add("family kinds", rays, [family_code(n, m, a, (b + 1) % P, True) for a, b in zip(i, kk)], 0)
    add("family kinds", rays, [family_code(n, m, (a + 1) % n, b, True) for a, b in zip(i, kk)], 0)

    # the lean twin's sign: dot(o - c_i, d) exactly 0, -0.0, +-tiny, NaN
    tangent = [[0.0, 1.0, 0.0], [-0.0, -1.0, -0.0], [1e-300, 1.0, 0.0], [-1e-300, 1.0, 0.0], [np.nan, 1.0, 0.0], [0.0, 0.0, 1.0], [-0.0, 0.0, -1.0]]
    tangent += [list(_unit(np.array([s * 2.0 ** -j, 1.0, 0.0]))) for j in (30, 45, 52, 60, 200) for s in (1.0, -1.0)]
    for i in range(min(n, 40)):
        o = sph[i, :3] + np.array([sph[i, 3] * (1.0 + 1e-6), 0.0, 0.0])
        add("lean twin", np.concatenate([np.tile(o, (len(tangent), 1)), np.array(tangent)], axis=1), 2 + i, 0)

    # NaN and inf in an origin or a direction, the zero direction
    i, rays = sphere_rays(6 * 3 + 1)
    bad = rays.copy()
    for j in range(6):
        for k, value in enumerate((np.nan, np.inf, -np.inf)):
            bad[3 * j + k, j] = value
    bad[-1, 3:] = 0.0
    add("non-finite", bad, 2 + i, 0)
    bad = bad.copy()
    bad[:, :3] = np.where(np.isfinite(bad[:, :3]), eyes[0], bad[:, :3])
    add("non-finite", bad, 0, 0)

    cls, rays, codes, frames = (np.concatenate([p[j] for p in parts]) for j in range(4))
    return {"rays": rays, "codes": codes, "frames": frames, "cls": cls, "aim": aim}


# ---- inputs: shadow-ray origins ----

@functools.lru_cache(maxsize=None)
def light_host(n, gi, li):
    sc = scene(n)
    gd, gp, depth = LIGHT_GRIDS[gi]
    kind, v, g = (0, -sc.dir_lights[li, :3], gd) if li < 2 else (1, sc.point_lights[li - 2, :3], gp)
    return lightlib().light_host_build(_f64(sc.spheres).ctypes.data, n, kind, _f64(v).ctypes.data, g, depth)


def light_lookup(n, gi, li, origins):
    """the host's own look-up: far, cell, lo, hi"""
    o = _f64(origins).reshape(-1, 3)
    far, cell, lo, hi = np.zeros(len(o), dtype=np.int32), np.zeros(len(o), dtype=np.int32), np.zeros(len(o)), np.zeros(len(o))
    lightlib().light_host_lookup(light_host(n, gi, li), o.ctypes.data, len(o), far.ctypes.data, cell.ctypes.data, lo.ctypes.data, hi.ctypes.data, None)
    return {"far": far, "cell": cell, "lo": lo, "hi": hi}


def light_coords(n, gi, li, cell):
    cell = _i32(cell)
    out = np.zeros((len(cell), 4), dtype=np.int32)
    lightlib().light_host_coords(light_host(n, gi, li), cell.ctypes.data, len(cell), out.ctypes.data)
    return out


def light_check(n, gi, li, origins, cell):
    """lightgrid_check.c's conservativeness and decision checks of the shadow rays from `origins` on the cells given (-1: not looked up)"""
    sc, o, cell = scene(n), _f64(origins).reshape(-1, 3), _i32(cell)
    st, any_st = LG.Stats(), LG.AnyHitStats()
    lightlib().lightgrid_check_at(light_host(n, gi, li), _f64(sc.spheres).ctypes.data, o.ctypes.data, cell.ctypes.data, len(o), C.byref(st))
    if li >= 2:
        lightlib().pointgrid_anyhit_check_at(light_host(n, gi, li), _f64(sc.spheres).ctypes.data, _f64(sc.ground).ctypes.data, o.ctypes.data, cell.ctypes.data,
                                             len(o), C.byref(any_st))
    return st, any_st


@functools.lru_cache(maxsize=None)
def light_inputs(n, gi, li):
    """origins [N, 3], class (index into LIGHT_CLASSES), the bisected pairs' host cells"""
    rng = np.random.default_rng(100 * n + 10 * gi + li)
    sc = scene(n)
    sph = sc.spheres
    rnge = np.zeros(4)
    lightlib().light_host_range(light_host(n, gi, li), rnge.ctypes.data)
    centre, rg = rnge[:3], np.sqrt(rnge[3])
    q = (100000 if n == 300 else 200000) - 35000
    parts, pairs = [], {}

    def add(cls, o):
        o = _f64(o).reshape(-1, 3)
        parts.append((np.full(len(o), LIGHT_CLASSES.index(cls), dtype=np.int32), o))

    def cell_of(o):
        got = light_lookup(n, gi, li, o)
        return np.where(got["far"] != 0, -1, got["cell"])

    # random: in the scene's box, in the shadow of a sphere, and out to beyond the table's range
    box = rng.uniform(-6.0, 6.0, (q // 2, 3))
    j = rng.integers(n, size=q // 2 - q // 10)
    away = np.tile(_unit(sc.dir_lights[li, :3]), (len(j), 1)) if li < 2 else _unit(sph[j, :3] - sc.point_lights[li - 2, :3])
    behind = sph[j, :3] + sph[j, 3:4] * rng.uniform(-1.0, 1.0, (len(j), 3)) + away * rng.uniform(0.3, 4.0, (len(j), 1))
    wide = centre + _rand_unit(rng, q // 10) * (rg * 10.0 ** rng.uniform(-3.0, 0.2, (q // 10, 1)))
    add("random", np.concatenate([box, behind, wide]))

    # origins across columns, rows and slabs (cells and shells) of the table
    def make(rng, k):
        a = rng.uniform(-5.0, 5.0, (k, 3))
        return a, a + rng.uniform(-1.5, 1.5, (k, 3))

    def looked_up(rng, k):
        a, b = make(rng, k)
        keep = (cell_of(a) >= 0) & (cell_of(b) >= 0)
        return a[keep], b[keep]
    a, b = bisect(*differing_pairs(rng, 2000, looked_up, cell_of), cell_of)
    for k, lo, hi in straddle(a, b):
        pairs[k] = (cell_of(lo), cell_of(hi))
        add("cell edges", np.concatenate([lo, hi]))

    # cube edges and corners about the light (for a directional light: about the look-up's centre), the centre itself, the spheres' centres
    v = special_vectors()
    add("cube edges", np.concatenate([centre + v * s for s in (1.0, 3.7, 0.01)] + [centre[None, :], sph[:, :3]]))
    # r2 either side of rg2
    e = np.array([s * x for x in (6e-8, 1.2e-7, 1e-6, 1e-3) for s in (1.0, -1.0)])
    u = _rand_unit(rng, 300)
    add("thresholds", np.concatenate([centre + u * (rg * (1.0 + x)) for x in e]))
    bad = rng.uniform(-3.0, 3.0, (9, 3))
    for j in range(3):
        for k, value in enumerate((np.nan, np.inf, -np.inf)):
            bad[3 * j + k, j] = value
    add("non-finite", bad)
    return {"origins": np.concatenate([p[1] for p in parts]), "cls": np.concatenate([p[0] for p in parts]), "pairs": pairs}


# ---- the CPU layer: the inputs are aimed ----

def own_place(host):
    """the place the host reads, -1 where the ray is no member (or has no family)"""
    read = host["member"] == 1
    return np.where(read, host["region"], -1), np.where(read, host["table"], -1), np.where(read, host["cell"], -1)


@pytest.mark.parametrize("m", PATCHES)
@pytest.mark.parametrize("n", COUNTS)
def test_path_inputs_are_aimed_and_the_hosts_own_lookups_are_conservative(n, m):
    inp = path_inputs(n, m)
    rays, codes, frames, aim = inp["rays"], inp["codes"], inp["frames"], inp["aim"]
    assert 150000 <= len(rays) <= 260000
    P = 6 * m * m if m else 1
    # bisected pairs: the host's cell differs between the -k and the +k member
    for key, (lo, hi) in aim["pairs"].items():
        assert (lo != hi).mean() >= 0.9, (key, (lo != hi).mean())
    assert len(aim["pairs"]) == (12 if m else 8)
    assert aim["patches seen"] == (set(range(P)), set(range(P))), "every patch, by the origin and by the mirror code"
    host = host_lookup(n, m, rays, codes, frames)
    # every membership threshold has members and non-members of the family it was made for
    for what, made in aim["thresholds"].items():
        member = np.concatenate([members_of(n, m, rays[sl], np.full(sl.stop - sl.start, region), np.full(sl.stop - sl.start, table)) for sl, region, table in made])
        assert 0.05 < member.mean() < 0.95, (what, member.mean())
        for sl, region, table in made:  # ... and the host looks the rays up in that family (the sphere's own: in it or in its twin)
            named = host["table"][sl] == table
            assert named.mean() > 0.95 and (host["region"][sl][named] >= region).all(), (what, region, table, named.mean())
    # the host checker on the host's own cells: nothing, and not vacuously -- per table kind
    region, table, cell = own_place(host)
    kinds = {"eye": (region == 0) & (table % 2 == 0), "mirror eye": (region == 0) & (table % 2 == 1), "sphere": (region == 1) & (table < n * P),
             "mirror sphere": (region == 1) & (table >= n * P), "lean twin": region == 2}
    for name, sel in kinds.items():
        st = judge(n, m, rays[sel], region[sel], table[sel], cell[sel])
        assert (st.violations, st.no_place, st.strangers) == (0, 0, 0), (name, st.violations, list(st.first_violation))
        assert st.exact_hits >= 1000 and st.judged >= 1000, (name, st.exact_hits, st.judged)
        if name == "lean twin":
            assert st.lean_reads == st.judged and st.lean_misses_own == st.lean_reads  # the own sphere's test misses wherever the twin is read
        if name == "sphere":
            assert st.full_hits_own >= 1000  # rays that go into their own sphere are answered from the full list
    assert set(frames.tolist()) == set(FRAMES) and (host["member"][inp["cls"] == CLASSES.index("family kinds")] == 0).mean() > 0.5
    lean = inp["cls"] == CLASSES.index("lean twin")
    assert {0, 1} <= set(host["lean"][lean].tolist()) and (host["member"][lean] == 1).mean() > 0.6


@pytest.mark.parametrize("gi", range(len(LIGHT_GRIDS)))
@pytest.mark.parametrize("n", COUNTS)
def test_shadow_inputs_are_aimed_and_the_hosts_own_lookups_are_conservative(n, gi):
    for li in range(4):
        inp = light_inputs(n, gi, li)
        o = inp["origins"]
        assert (80000 if n == 300 else 180000) <= len(o) <= 230000
        for k, (lo, hi) in inp["pairs"].items():
            assert (lo != hi).mean() >= 0.9, (li, k, (lo != hi).mean())
        host = light_lookup(n, gi, li, o)
        thr = inp["cls"] == LIGHT_CLASSES.index("thresholds")
        assert 0.2 < host["far"][thr].mean() < 0.8, "r2 either side of rg2"
        st, any_st = light_check(n, gi, li, o, np.where(host["far"] != 0, -1, host["cell"]))
        assert (st.violations, st.decision_mismatches, any_st.wrong_dark, any_st.wrong_lit) == (0, 0, 0, 0), (li, st.violations, list(st.first_violation))
        assert st.exact_hits >= 1000 and st.rays - st.far >= 40000, (li, st.exact_hits, st.far)
        if li >= 2:
            assert any_st.dark >= 1000 and any_st.lit >= 1000, (li, any_st.dark, any_st.lit)


# ---- the filter's inputs ----

def filter_rays(n):
    """the path rays above (fewer in the large scenes: the sign words are rays x spheres)"""
    rays = path_inputs(n, 0)["rays"]
    return rays[::max(1, (len(rays) * n) // 6000000)]


def filter_host(sc, rays):
    rays, sph = _f64(rays), _f64(sc.spheres)
    n = len(sph)
    fields, sign, fixed = np.zeros((len(rays), 9), dtype=np.uint32), np.zeros((n, len(rays)), dtype=np.uint32), np.zeros((n, len(rays)), dtype=np.uint32)
    lightlib().filter_host_words(sph.ctypes.data, n, rays.ctypes.data, len(rays), _f64(sc.dir_lights[0, :3]).ctypes.data, fields.ctypes.data, sign.ctypes.data,
                                 fixed.ctypes.data)
    return fields, sign, fixed


def scaled(sc, rays, scale):
    """the scene and the rays' origins in other units"""
    sph = sc.spheres.copy()
    sph[:, :4] *= scale
    rays = rays.copy()
    rays[:, :3] *= scale
    return S.SceneData(sph, sc.ground, sc.dir_lights, sc.point_lights, sc.camera, sc.sky), rays


FILTER_SCALES = (1e-18, 1e18, 1e20)  # at 1e+18 the bounds of these scenes (8 units across) stay just inside FP32: 1e+20 is where they overflow


def test_filter_inputs_reach_denormal_and_overflowing_intermediates():
    """at 1e-18 the filter's FP32 bounds are denormal, at 1e+18 they are within a factor of a few of FLT_MAX, at 1e+20 they overflow and the ray is not ok"""
    sc = scene(70)
    rays = filter_rays(70)[::10]
    fields, _, _ = filter_host(sc, rays)
    assert (fields[:, 8] == 1).sum() > 1000 and (fields[:, 8] == 0).sum() > 50
    small, _, _ = filter_host(*scaled(sc, rays, 1e-18))
    # E >= 40 eps Wn^2 and E <= 40 eps (Cn + Wn + Rm)^2 + ..., Cn + Rm < 9e-18 here: an FP32 denormal that is not zero
    wn = np.abs(small[:, 3:6].view(np.float32)).astype(np.float64).sum(axis=1)
    denormal = (40 * 2.0 ** -24 * wn ** 2 > 1.5e-45) & (41 * 2.0 ** -24 * (wn + 9e-18) ** 2 < 1.17549435e-38)
    assert denormal.sum() > 1000 and (small[denormal, 8] == 1).sum() > 1000
    large, _, _ = filter_host(*scaled(sc, rays, 1e18))
    thr = np.abs(large[:, 6].view(np.float32))
    assert ((thr > 1e36) & np.isfinite(thr)).sum() > 1000 and np.array_equal(large[:, 8], fields[:, 8])
    larger, _, _ = filter_host(*scaled(sc, rays, 1e20))
    assert (larger[:, 8] == 0).mean() > 0.5 and (larger[:, 8] == 1).sum() > 10  # |O'|^2 overflows unless the line passes near the scene's middle


# ---- the GPU layer ----

def per_class(names, cls, differ, looked_up):
    return {name: (int(differ[cls == j].sum()), int(looked_up[cls == j].sum())) for j, name in enumerate(names) if (cls == j).any()}


def check_path_lookups(n, m, inp, frames, dev, pool, tag):
    """A to D for one call of trt_probe_path_lookups; returns {class: (look-ups that differ from the host's, look-ups)}"""
    rays, codes, cls = inp["rays"], inp["codes"], inp["cls"]
    P, (ge, gs) = (6 * m * m if m else 1), PATH_GRIDS[n]
    host = host_lookup(n, m, rays, codes, frames)
    valid, read = host["region"] >= 0, dev["read_at"] >= 0  # a code the kernel can decode | the device read a cell
    # D: a ray without a family reads nothing, falls back and has no successor
    assert not read[~valid].any() and (dev["fallback"][~valid] == 1).all() and (dev["successor"][~valid] == -1).all(), tag
    assert (dev["region"][read] >= 0).all() and (dev["region"][~read] == -1).all() and (dev["word"][~read] == 0).all(), tag
    # The table the device uses is named by the code and the frame -- and, for a ray from a sphere with patches, by the patch the device chose, which
    # the successor code carries.
    own = valid & (codes >= 2) & (codes < 2 + n)
    k_dev = host["patch"].copy()
    if m:
        rest = dev["successor"][own] - 2 - n
        assert ((rest >> SHIFT) == codes[own] - 2).all() and ((rest & 127) < P).all(), tag
        k_dev[own] = rest & 127
        want = np.where(codes == 0, 1, np.where(own, dev["successor"], -1))
    else:
        want = codes
    assert np.array_equal(dev["successor"][valid], want[valid]), (tag, "D: the successor code")
    named_region, named_table = host["region"], host["table"] + np.where(own, k_dev - host["patch"], 0)
    # A: the membership verdict is the host's, for the table the device used
    member = members_of(n, m, rays, named_region, named_table) == 1
    bad = np.nonzero(valid & (read != member))[0]
    assert not len(bad), (tag, "A: membership", len(bad), rays[bad[:3]], codes[bad[:3]])
    # D: the eye slot of the frame, the mirror block, the patch, the twin exactly where the ray leaves its own sphere outwards
    bad = np.nonzero(read & ((dev["region"] != named_region) | (dev["table"] != named_table)))[0]
    assert not len(bad), (tag, "D: the table", len(bad), dev["region"][bad[:5]], dev["table"][bad[:5]], named_region[bad[:5]], named_table[bad[:5]])
    assert (dev["region"][read] == 2).sum() >= 1000 and ((dev["region"] == 1) & (dev["table"] < n * P))[read].sum() >= 1000, tag
    # B: the face is the host's, column and row the host's or a neighbour's -- of the cell and of the patch
    g = np.where(named_region == 0, ge, gs)
    for what, sel, mine, theirs, side in (("cell", read, dev["cell"], host["cell"], g), ("patch", own & (m > 0), k_dev, host["patch"], np.full(len(g), max(m, 1)))):
        (f0, r0, c0), (f1, r1, c1) = face_row_col(mine, side), face_row_col(theirs, side)
        bad = np.nonzero(sel & ((f0 != f1) | (np.abs(r0 - r1) > 1) | (np.abs(c0 - c1) > 1)))[0]
        assert not len(bad), (tag, "B: beyond a neighbour", what, len(bad), rays[bad[:3]], mine[bad[:3]], theirs[bad[:3]])
    differ = read & ((dev["cell"] != host["cell"]) | (named_table != host["table"]))
    counts = per_class(CLASSES, cls, differ, read)
    assert counts["random"][1] >= 50000 and counts["random"][0] <= 1e-4 * counts["random"][1], (tag, "B: random rays", counts)
    # D: a ray falls back exactly when it is no member of that table or the cell has no list
    none = (dev["word"] >> np.uint64(56)) == 0xFF
    assert np.array_equal(dev["fallback"] == 1, ~read | none), (tag, "D: fallback")
    # C: the host's conservativeness check on the device's place, and the device's cell word against the host's table at that place
    st = judge(n, m, rays, dev["region"], dev["table"], dev["cell"])
    assert (st.violations, st.no_place, st.strangers) == (0, 0, 0), (tag, "C", st.violations, st.no_place, st.strangers, list(st.first_violation))
    assert st.exact_hits >= 5000 and st.judged == read.sum() - st.no_list, tag
    pool = np.ascontiguousarray(pool, dtype=np.uint64)
    region, table, cell, words = _i32(dev["region"]), _i32(dev["table"]), _i32(dev["cell"]), np.ascontiguousarray(dev["word"], dtype=np.uint64)
    wrong = pathlib().lookup_path_same_entries(path_host(n, m), region.ctypes.data, table.ctypes.data, cell.ctypes.data, words.ctypes.data, pool.ctypes.data,
                                               len(pool), len(words))
    assert wrong == 0, (tag, "C: cell words that list something else than the host's table", wrong)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("m", PATCHES)
@pytest.mark.parametrize("n", COUNTS)
def test_the_devices_path_lookups_read_where_the_hosts_proofs_hold(n, m):
    """trt_probe_path_lookups -- the render kernels' own path_cell / path_cell_patches on the image a frame stages -- for one camera and for a batch of
    eight whose eyes differ, rays of frames 0, 1 and 7: A to D of this file's head"""
    inp, cams = path_inputs(n, m), cameras()
    with hip.Context(0) as ctx:
        ctx.set_path_grids_min_spheres(0)
        ctx.set_light_grids(0, 0)
        ctx.set_path_patches(m)
        ctx.set_path_grids(*PATH_GRIDS[n])
        ctx.set_path_lean_lists(1)
        ctx.set_scene(scene(n))
        assert ctx.path_patches() == (m, 6 * m * m if m else 1) and ctx.path_lean_lists()["in_use"]
        single = ctx.probe_path_lookups(cams[0], inp["rays"], inp["codes"])
        batch = ctx.probe_path_lookups(cams, inp["rays"], inp["codes"], inp["frames"])
        info, _, pool = ctx.read_path_tables(cams[0])  # the whole pool: the scene's part, the twins' lists, every eye slot's
        assert info["enabled"] == 1 and (info["eye_cells"], info["sphere_cells"]) == PATH_GRIDS[n]
    for tag, dev, frames in (("one camera", single, np.zeros(len(inp["rays"]), dtype=np.int32)), ("batch of 8", batch, inp["frames"])):
        counts = check_path_lookups(n, m, inp, frames, dev, pool, (n, m, tag))
        print(f"path look-ups n={n} m={m} {tag}: differing from the host's / looked up per class: {counts}")
    eye = inp["codes"] < 2
    assert set((batch["table"][eye & (batch["read_at"] >= 0)] // 2).tolist()) == set(FRAMES)  # slot b for frame b


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(LIGHT_GRIDS)), ids=["%dx%d, depth %d" % g for g in LIGHT_GRIDS])
@pytest.mark.parametrize("n", COUNTS)
def test_the_devices_shadow_lookups_read_where_the_hosts_proofs_hold(n, gi):
    """trt_probe_shadow_lookups -- the shading stage's look-up lines on the staged headers -- for the two directional and the two point lights"""
    gd, gp, depth = LIGHT_GRIDS[gi]
    sc = scene(n)
    with hip.Context(0) as ctx:
        ctx.set_path_grids(0, 0)
        ctx.set_light_slabs(depth, depth)
        ctx.set_light_grids(gd, gp)
        ctx.set_scene(sc)
        got = [(ctx.probe_shadow_lookups(light_inputs(n, gi, li)["origins"], li), ctx.read_light_lists(int(li >= 2), li % 2)) for li in range(4)]
    for li, (dev, (info, cells, pool)) in enumerate(got):
        inp = light_inputs(n, gi, li)
        o, cls, tag = inp["origins"], inp["cls"], (n, LIGHT_GRIDS[gi], "light", li)
        host = light_lookup(n, gi, li, o)
        assert info["enabled"] == 1 and info["cells"] == depth * (gd * gd if li < 2 else 6 * gp * gp)
        # A: far, and a directional light's cell
        assert np.array_equal(dev["far"] != 0, host["far"] != 0), (tag, "A: far")
        near = host["far"] == 0
        assert near.sum() >= 40000 and (dev["word"][~near] == 0).all() and ((dev["cell"][near] >= 0) & (dev["cell"][near] < info["cells"])).all(), tag
        differ = near & (dev["cell"] != host["cell"])
        if li < 2:
            assert not differ.any(), (tag, "A: trt_dirgrid_cell", int(differ.sum()), o[differ][:3])
        else:
            # A: the bounds of the any-hit search, as bits
            for name in ("lo", "hi"):
                bad = np.nonzero(near & (T.bits(dev[name]) != T.bits(host[name])))[0]
                assert not len(bad), (tag, "A: " + name, len(bad), o[bad[:3]], dev[name][bad[:3]], host[name][bad[:3]])
            # B: the face is the host's; shell, row and column the host's or a neighbour's
            mine, theirs = light_coords(n, gi, li, np.where(near, dev["cell"], 0)), light_coords(n, gi, li, np.where(near, host["cell"], 0))
            bad = np.nonzero(near & ((mine[:, 1] != theirs[:, 1]) | (np.abs(mine - theirs) > 1).any(axis=1)))[0]
            assert not len(bad), (tag, "B: beyond a neighbour", len(bad), o[bad[:3]], mine[bad[:3]], theirs[bad[:3]])
        counts = per_class(LIGHT_CLASSES, cls, differ, near)
        assert counts["random"][0] <= 1e-4 * counts["random"][1], (tag, "B: random origins", counts)
        print(f"shadow look-ups n={n} grids={LIGHT_GRIDS[gi]} light {li}: differing from the host's / looked up per class: {counts}")
        # C: the host's checks on the device's cell; the word read there lists the spheres of the host's mask
        assert np.array_equal(dev["word"][near], cells[dev["cell"][near]]), tag
        st, any_st = light_check(n, gi, li, o, np.where(near, dev["cell"], -1))
        assert (st.violations, st.decision_mismatches, any_st.wrong_dark, any_st.wrong_lit) == (0, 0, 0, 0), (tag, "C", st.violations, list(st.first_violation))
        assert st.exact_hits >= 1000, tag
        cell, words = _i32(np.where(near, dev["cell"], -1)), np.ascontiguousarray(dev["word"], dtype=np.uint64)
        pool = np.ascontiguousarray(pool, dtype=np.uint64)
        wrong = lightlib().light_host_same_entries(light_host(n, gi, li), cell.ctypes.data, words.ctypes.data, pool.ctypes.data, len(pool), info["list_bits"], len(words))
        assert wrong == 0, (tag, "C: cell words that list something else than the host's mask", wrong)


def same_floats(a, b):
    """equal bit for bit; two NaNs are equal whatever their sign and payload"""
    fa, fb = a.view(np.float32), b.view(np.float32)
    return (a == b) | (np.isnan(fa) & np.isnan(fb))


@pytest.mark.gpu
@pytest.mark.parametrize("n", COUNTS)
def test_the_devices_filter_words_are_the_hosts(n):
    """trt_selftest_filter: trt_filter_setup's nine fields, the sign word of every sphere and the fixed-direction sign words of directional light 0, on
    the path rays of this file, and in scenes scaled by 1e-18 (FP32 intermediates go denormal), 1e+18 (they come within a factor of a few of FLT_MAX) and 1e+20
    (they overflow: ok = 0)"""
    base, rays = scene(n), filter_rays(n)
    not_ok = {}
    with hip.Context(0) as ctx:
        ctx.set_path_grids(0, 0)
        ctx.set_light_grids(0, 0)
        for scale in (1.0,) + FILTER_SCALES:
            sc, scaled_rays = scaled(base, rays, scale)
            ctx.set_scene(sc)
            fields, sign, fixed = ctx.selftest_filter(scaled_rays, n)
            want_fields, want_sign, want_fixed = filter_host(sc, scaled_rays)
            tag = (n, scale)
            bad = np.nonzero(~same_floats(fields[:, :8], want_fields[:, :8]).all(axis=1) | (fields[:, 8] != want_fields[:, 8]))[0]
            assert not len(bad), (tag, "A: trt_filter_setup", len(bad), scaled_rays[bad[:3]], fields[bad[:3]], want_fields[bad[:3]])
            ok = want_fields[:, 8] == 1
            not_ok[scale] = int((~ok).sum())
            assert ok.sum() > 10, tag
            for name, got, want in (("trt_filter_sign", sign, want_sign), ("trt_filter_sign_fixed_dir", fixed, want_fixed)):
                if scale < 1e19:  # (at 1e+20 the culling table itself holds inf and NaN)
                    assert np.array_equal(got[:, ok], want[:, ok]), (tag, "A: " + name, int((got[:, ok] != want[:, ok]).sum()))
                assert same_floats(got, want).all(), (tag, "A: " + name + ", NaN for NaN", int((~same_floats(got, want)).sum()))
    assert not_ok[1e20] > len(rays) // 2 > not_ok[1e18], not_ok  # at 1e+20 the bounds of most rays overflow
