"""LEAN TWINS of the spheres' own families on the device (csrc/trt_raygrid.h, csrc/trt_tables.hip, path_cell in
csrc/trt_rounds.hpp; the host layer is tests/test_lean_lists.py): the twins the device derives equal the host's derivation,
frames and ray counts do not depend on the switch (trt_set_path_lean_lists) and stay the oracle's in the plain, the decoupled
and the patch variants, probe rays aimed inwards still find their own sphere, and the counting variant shows what the twins
are for: fewer iterations of the path rays' exact loop, nothing else changed."""
import ctypes as C

import numpy as np
import pytest

import support as T
from support import COMPACT, PLAIN, bits
from terminalraytracer_amd import hip
from terminalraytracer_amd import scenes as S
import test_lean_lists as H

pytestmark = pytest.mark.gpu

PATCHES = "patches"  # the patch instantiation (24 or 6 patches per sphere), whatever the number of spheres
VARIANTS = [PLAIN, COMPACT, PATCHES]


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def checker():
    return H.build_checker()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield
    if "ctx" in request.fixturenames:
        c = request.getfixturevalue("ctx")
        c.enable_counters(False)
        c.set_refraction(None)
        c.set_list_pool_words(0)
        c.set_path_grids(64, 32)
        c.set_path_patches(-1)
        c.set_path_grids_min_spheres(12)
        c.set_compaction(-1)
        c.set_path_lean_lists(-1)


def select(ctx, variant, patch_m=1):
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_compaction(1 if variant == COMPACT else 0 if variant == PLAIN else -1)
    ctx.set_path_patches(patch_m if variant == PATCHES else 0)
    ctx.set_path_grids_min_spheres(0)


def loop_counts(ctx):
    """trt_read_loop_diagnostics as it comes: wave-level iterations of the three exact loops, then the lanes' exact tests in them"""
    raw = (C.c_ulonglong * 8)()
    assert hip.lib().trt_read_loop_diagnostics(ctx._h, raw) == 0
    return [int(x) for x in raw]


def both_ways(ctx, scene, w, h, b, spp, cameras=None, count=True):
    """the frame(s), the counters and the diagnostics with the twins off and on; with the switch on the look-ups must read twins"""
    out = []
    ctx.enable_counters(count)
    for mode in (0, 1):
        ctx.set_path_lean_lists(mode)
        ctx.set_scene(scene)
        assert ctx.path_lean_lists()["in_use"] == bool(mode)
        rows = hip.RowSet.whole(w, h)
        got = ctx.render_host(scene.camera, rows, b, spp) if cameras is None else ctx.render_host_batch(cameras, rows, b, spp)
        out.append((got, ctx.read_counters(), dict(ctx.read_diagnostics(), loops=loop_counts(ctx))) if count else (got, None, None))
    return out


# ---- the device's twins ----

@pytest.mark.parametrize("name,make,grids", H.SMALL, ids=[s[0] for s in H.SMALL])
def test_device_twins_equal_the_host_derivation(ctx, checker, name, make, grids):
    scene = make()
    n = len(scene.spheres)
    bits_per = 16 if n > 256 else 8
    ctx.set_path_grids_min_spheres(0)
    ctx.set_path_lean_lists(1)
    for g_eye, g_sph, m in grids + [(8, 16, 0)]:
        for cap in (0, 64):  # 64 words: the scene's part of the pool is exhausted before the twins ask
            ctx.set_list_pool_words(cap)
            ctx.set_path_grids(g_eye, g_sph)
            ctx.set_path_patches(m)
            ctx.set_scene(scene)
            info, cells, pool = ctx.read_path_tables(scene.camera)
            lean = ctx.read_path_lean_tables()
            P = 6 * m * m if m else 1
            table_cells = 6 * g_sph * g_sph
            count = n * P * table_cells
            full = np.ascontiguousarray(cells[2 * 6 * g_eye * g_eye:][:count])
            assert lean.size == count and ctx.path_lean_lists() == {"in_use": True, "twin_bytes": 8 * count}
            # every twin is its full cell minus the own sphere (with a capped pool: or a copy of it) ...
            st = H.Stats()
            checker.lean_compare(full.ctypes.data, lean.ctypes.data, count, table_cells, P, pool.ctypes.data, bits_per, int(cap != 0), C.byref(st))
            print(f"\n{name} g {g_sph} m {m} cap {cap}: stripped {st.stripped} no list {st.no_list} pooled -> inline {st.now_inline} "
                  f"still pooled {st.still_pooled} copies {st.copies}")
            assert st.violations == 0, list(st.first_violation)
            assert st.stripped + st.copies + st.no_list == count and st.unchanged == st.no_list
            assert cap or (st.no_list == 0 and st.copies == 0)
            # ... and what the header's function derives on the host from the same full cells
            if cap == 0:
                host = np.zeros_like(lean)
                words = np.concatenate([pool, np.zeros(pool.size + 16, dtype=np.uint64)])
                used = C.c_long(pool.size)
                checker.lean_derive(full.ctypes.data, host.ctypes.data, count, table_cells, P, words.ctypes.data, C.byref(used), words.size, bits_per, C.byref(st))
                assert st.violations == 0
                assert checker.lean_same_entries(lean.ctypes.data, pool.ctypes.data, host.ctypes.data, words.ctypes.data, count, bits_per) == 0
                # the twins' long lists lie in the scene's part of the pool, behind no one else's
                at = [int(x) & 0xFFFFFFFF for x in lean if (int(x) >> 56) == 0x80]
                assert all(a < info["pool_used_scene"] for a in at)


def test_the_switch_and_the_memory():
    """-1 and 1: twins, built when the scene has none; 0: the full tables.  Their bytes are part of trt_scene_info's, the tables trt_read_path_tables reports are the same either way."""
    with hip.Context(0) as ctx:  # a context of its own: a context's buffers only grow, and the bytes are what this is about
        scene = S.synth_scene(64, T.sky("synth"), T.bench_camera(64, 36))
        ctx.set_path_lean_lists(0)
        ctx.set_scene(scene)
        without = ctx.scene_info()["table_bytes"]
        info0, cells0, pool0 = ctx.read_path_tables(scene.camera)
        assert ctx.path_lean_lists() == {"in_use": False, "twin_bytes": 0} and ctx.read_path_lean_tables().size == 0
        builds = ctx.build_counts()[0]
        ctx.set_path_lean_lists(-1)  # on: the scene in place is built again, with twins
        assert ctx.build_counts()[0] == builds + 1
        twins = 8 * 64 * 6 * 32 * 32
        assert ctx.path_lean_lists() == {"in_use": True, "twin_bytes": twins}
        assert ctx.scene_info()["table_bytes"] >= without + twins
        info1, cells1, pool1 = ctx.read_path_tables(scene.camera)
        assert info1["cells"] == info0["cells"] and checker_same(cells0, pool0, cells1, pool1)
        ctx.set_path_lean_lists(0)   # off again: nothing is built, the look-ups read the full tables
        assert ctx.build_counts()[0] == builds + 1 and not ctx.path_lean_lists()["in_use"]
        ctx.set_path_lean_lists(1)
        assert ctx.build_counts()[0] == builds + 1 and ctx.path_lean_lists()["in_use"]
        ctx.set_scene(scene)         # the same scene, the same settings: no build
        assert ctx.build_counts()[0] == builds + 1
        ctx.set_path_lean_lists(-1)
        ctx.set_path_patches(1)      # six patches per sphere: six times the twins
        assert ctx.path_lean_lists() == {"in_use": True, "twin_bytes": 6 * twins}
        with hip.Context(0) as other:  # tables shared with another context are not rebuilt under it
            ctx.set_path_lean_lists(0)
            ctx.set_scene(scene)
            other.share_scene(ctx)
            with pytest.raises(hip.TrtError):
                other.set_path_lean_lists(1)
            assert not other.path_lean_lists()["in_use"]


def checker_same(cells_a, pool_a, cells_b, pool_b):
    lib = H.build_checker()
    return cells_a.size == cells_b.size and lib.lean_same_entries(cells_a.ctypes.data, pool_a.ctypes.data, cells_b.ctypes.data, pool_b.ctypes.data,
                                                                  cells_a.size, 8) == 0


# ---- frames ----

def grazing_scene():
    """one large mirror sphere whose surface the eye all but touches: it fills the view out to its horizon, where the primary rays
    graze it and the reflected rays leave it nearly tangentially; the other spheres are inside it, cut it or peep over its horizon"""
    base = S.synth_scene(16, T.sky("synth"), T.bench_camera(96, 54, 2.5), seed=9)
    sph = base.spheres.copy()
    sph[0, 3] = 0.97 * np.linalg.norm(base.camera[9:12] - sph[0, :3])
    sph[0, 7] = 0.9
    return base.with_spheres(sph)


def nested_scene():
    base = S.synth_scene(40, T.sky("synth"), T.bench_camera(64, 36, 10.0), seed=5)
    odd = base.spheres.copy()
    odd[2, :3] = odd[3, :3] + [odd[3, 3] + odd[2, 3], 0.0, 0.0]  # touching
    odd[4, :4] = odd[5, :4]                                       # duplicates: the same centre, the same radius
    odd[6, :3] = odd[7, :3]
    odd[6, 3] = odd[7, 3] * 0.5                                   # nested: the same centre, half the radius
    odd[8, :3] = odd[9, :3]
    odd[8, 3] = odd[9, 3] * (1.0 + 1e-9)                          # a shell a hair outside another sphere
    odd[1, 3] = 5e-5                                              # a radius below 1e-4
    odd[:, 7] = np.where(np.arange(len(odd)) % 2 == 0, 1.0, odd[:, 7])
    return base.with_spheres(odd)


def mixed_scene():
    """mirrors and matt spheres side by side: after the first bounce a wave holds primary rays of fresh samples, rays that left a
    sphere outwards (twins), rays reflected by the ground (mirror families, full tables) and dead lanes at once"""
    return S.synth_scene(64, T.sky("synth"), T.bench_camera(80, 45), mirror_fraction=0.5)


FRAME_SCENES = [("grazing", grazing_scene, 96, 54, 8, 3), ("nested and touching", nested_scene, 64, 36, 8, 4), ("mixed wave", mixed_scene, 80, 45, 8, 3)]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name,make,w,h,b,spp", FRAME_SCENES, ids=[f[0] for f in FRAME_SCENES])
def test_frames_and_ray_counts_are_the_oracles_with_and_without_twins(ctx, name, make, w, h, b, spp, variant):
    scene = make()
    with np.errstate(all="ignore"):
        want, st = T.oracle_render(scene, w, h, b, spp)
    select(ctx, variant)
    (off, off_count, off_diag), (on, on_count, on_diag) = both_ways(ctx, scene, w, h, b, spp)
    assert variant == PATCHES or ctx.render_variant()["decoupled"] == (variant == COMPACT)
    assert ctx.path_patches()[0] == (1 if variant == PATCHES else 0)
    assert np.array_equal(bits(off), bits(want)) and np.array_equal(bits(on), bits(want))
    assert off_count == on_count == (st.path_rays, st.shadow_rays)
    print(f"\n{name} {variant}: exact-loop iterations of the path rays {off_diag['exact_loop_iterations']['path']} -> {on_diag['exact_loop_iterations']['path']}")
    # (not always fewer: a wave whose longest list falls from 13 entries to 12 loses the FP32 thinning of trace(), kListPrefilter, and
    # runs 12 exact tests where 13 thinned ones had left two or three -- the grazing scene, whose large sphere sits in every list)
    assert on_diag["swept_traces"] == off_diag["swept_traces"]  # no new fall-back to the sweep


def test_a_refraction_scene_against_its_restatement(ctx):
    """Rays inside a refractor meet their own sphere at the far root whatever the sign of b: they keep the full list."""
    base = S.synth_scene(24, T.sky("synth"), T.bench_camera(96, 54, 2.5), seed=3)
    sph = base.spheres.copy()
    sph[5, :3] = sph[4, :3]
    sph[5, 3] = sph[4, 3] * 0.5                                   # a sphere nested in a refractor
    sph[7, :3] = sph[6, :3] + [sph[6, 3] + sph[7, 3], 0.0, 0.0]  # touching
    scene = base.with_spheres(sph)
    ior = np.where(np.arange(24) % 3 == 0, 1.5, 0.0)
    ior[1], ior[2], ior[4], ior[7] = 0.7, 1.0, 1.33, 2.4
    w, h, b, spp = 96, 54, 10, 3
    want, st = T.oracle_render_refractive(scene, ior, w, h, b, spp)
    for patches in (0, 1):
        ctx.set_path_patches(patches)
        ctx.set_refraction(ior)
        (off, off_count, _), (on, on_count, _) = both_ways(ctx, scene, w, h, b, spp)
        assert np.array_equal(bits(off), bits(want)) and np.array_equal(bits(on), bits(want)), patches
        assert off_count == on_count == (st.path_rays, st.shadow_rays)


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_batch_of_two_cameras(ctx, variant):
    w, h, b, spp = 64, 36, 6, 3
    cams = np.stack([T.bench_camera(w, h, 1.0), T.bench_camera(w, h, 10.0)])
    scene = S.synth_scene(64, T.sky("synth"), cams[0])
    select(ctx, variant)
    (off, _, _), (on, _, _) = both_ways(ctx, scene, w, h, b, spp, cameras=cams, count=False)  # (a counted batch is served camera by camera)
    assert ctx.batch_info()[0] == 2
    for k, cam in enumerate(cams):
        want, _ = T.oracle_render(scene.with_camera(cam), w, h, b, spp)
        assert np.array_equal(bits(off[k]), bits(want)) and np.array_equal(bits(on[k]), bits(want)), k


# ---- single rays ----

@pytest.mark.parametrize("patches", [0, 1])
def test_probe_rays_aimed_inwards_find_their_own_sphere(ctx, patches):
    """Rays from 1e-6 outside the surface of sphere i, looked up in family 2 + i like a reflected ray, aimed at the sphere, past
    it and along its tangent plane: whatever reads a twin misses sphere i in the reference's test too -- the production stages
    answer every ray as the reference-order kernel does, and the rays aimed inwards return sphere i itself."""
    scene = nested_scene()
    sph = scene.spheres
    rng = np.random.default_rng(3)
    rays, own = [], []
    for i in (0, 3, 6, 7, 8, 9, 1):
        r = H.directed_rays(sph, i, rng)
        rays.append(r), own.append(np.full(len(r), i))
    rays, own = np.concatenate(rays), np.concatenate(own)
    ctx.set_path_grids_min_spheres(0)
    ctx.set_path_patches(patches)
    ctx.set_scene(scene)
    want = ctx.probe_rays(rays)  # the reference-order kernel: every sphere tested against every ray
    inwards = np.einsum("ij,ij->i", rays[:, :3] - sph[own, :3], rays[:, 3:]) < -0.4 * np.abs(sph[own, 3])  # at 27 degrees or more into the surface
    outside = np.linalg.norm(rays[:, :3] - sph[own, :3], axis=1) > np.abs(sph[own, 3]) + 5e-7
    for mode in (0, 1):
        ctx.set_path_lean_lists(mode)
        got = ctx.probe_rays_production(scene.camera, rays, (2 + own).astype(np.int32))
        assert np.array_equal(got[0], want[0]), mode
        for a, b_, what in zip(got[1:4], want[1:4], ("point", "normal", "material")):
            assert np.array_equal(bits(a), bits(b_)), (mode, what)
        hit = want[0] != 0
        assert np.array_equal(bits(got[4][hit]), bits(want[4][hit])), (mode, "lit")
        # aimed inwards from outside: the ray's own sphere, or a sphere nested in it / a duplicate of it with a lower index, is what it hits
        hit_own = np.isclose(np.linalg.norm(got[1] - sph[own, :3], axis=1), np.abs(sph[own, 3]), rtol=1e-6, atol=0.0)
        sel = inwards & outside & ~np.isin(own, (7, 9, 8))  # (7 and 9 hold a nested sphere / lie inside a shell; 8 is that shell)
        assert sel.sum() > 100 and hit_own[sel].all() and (got[0][sel] != 0).all()


# ---- what the twins are for ----

def test_the_counting_variant_shows_shorter_exact_loops_and_nothing_else(ctx):
    """BASELINE config 3's scene (64 spheres, 8 bounces) at 160 x 90: the exact loop of the path rays runs as long as the longest
    list among a wave's lanes, and the own sphere was in every list of a lane that had left a sphere."""
    scene = S.synth_scene(64, T.sky("synth"), T.bench_camera(160, 90))
    w, h, b, spp = 160, 90, 8, 10
    want, st = T.oracle_render(scene, w, h, b, spp)
    for variant in (PLAIN, COMPACT):
        select(ctx, variant, patch_m=0)
        ctx.set_path_grids_min_spheres(12)
        (off, off_count, d0), (on, on_count, d1) = both_ways(ctx, scene, w, h, b, spp)
        assert np.array_equal(bits(off), bits(want)) and np.array_equal(bits(on), bits(want))
        assert off_count == on_count == (st.path_rays, st.shadow_rays)
        trips = max(1, d0["wave_loop_trips"])
        l0, l1 = d0["loops"], d1["loops"]  # [0], [3]: the path loop's wave-level iterations and its lanes' exact tests
        print(f"\n{variant}: path exact-loop iterations per round {l0[0] / trips:.3f} -> {l1[0] / trips:.3f}, "
              f"lane tests per path ray {l0[3] / st.path_rays:.3f} -> {l1[3] / st.path_rays:.3f}")
        assert l1[0] < l0[0] and l1[3] < l0[3] and l0[1:3] == l1[1:3] and l0[4:] == l1[4:]
        print({k: (d0[k], d1[k]) for k in d0 if d0[k] != d1[k]})
        same = ("wave_loop_trips", "swept_traces", "shading_passes", "point_light_closest_hit_fallbacks")  # (phase2_rounds counts the path loop's iterations too)
        assert all(d0[k] == d1[k] for k in same), [(k, d0[k], d1[k]) for k in same]
        for kind in ("directional", "point"):
            assert d0["exact_loop_iterations"][kind] == d1["exact_loop_iterations"][kind]
            assert d0["exact_loop_lane_activity"][kind] == d1["exact_loop_lane_activity"][kind]
