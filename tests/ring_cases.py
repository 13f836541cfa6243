"""Directed launches for the decoupled rounds' task ring (tests/test_ring_model.py on the CPU, tests/test_decoupled_ring.py on the device).

Every frame is a fan of near-horizontal rays from an eye at the origin, one per column, looking down -z a little above the horizon:
a column that nothing covers meets the sky with its first ray.  What a column does is decided by the one sphere that covers it:

 dark   reflectivity 0: the sample ends on its first hit, by weight (by the limit at a bounce limit of 1);
 down   a mirror whose centre lies above the fan: the ray leaves it downwards and meets the ground -- a second hit, the last one on a
        dark ground; on a mirror ground it goes on upwards, into the sky or into a dark sphere that hangs over the whole scene;
 up     a mirror whose centre lies below the fan: the ray leaves it upwards, into the sky.

The spheres' places and radii were found on the CPU (each silhouette's edges half a column from the nearest ray) and are committed as
numbers; the scene is only a means.  tests/test_ring_model.py asserts, through the oracle's ray log and the model, that each launch
reaches the state it is named for, so that an edit here cannot lose the edge silently."""
import functools

import numpy as np

import ring_model as M
import support as T
from terminalraytracer_amd import scenes as S

CHUNK, CHUNK_SMALL, XCD_SHIFT, BLOCK, COMPACT_BLOCK = 256, 128, 3, 256, 1024  # asserted against the source by tests/test_ring_model.py

DIR_LIGHTS = np.array([[-0.3, -1.0, -0.5, 0.8, 0.7, 0.6]])
POINT_LIGHTS = np.array([[1.0, 6.0, 3.0, 0.6, 0.7, 0.9, 400.0]])
DARK, MIRROR = 0.0, 1.0

SPHERES = {
    "sky": [[50.0, 50.0, -10.0, 1.0, 0.9, 0.6, 0.3, 0.0, 100.0]],
    "s1": [[-0.01968, 0.1, -10.0, 1.26964, 0.9, 0.6, 0.3, 0.0, 100.0]],
    "s2": [[-0.05912, 1.03842, -10.0, 1.56404, 0.5, 0.8, 0.9, 1.0, 100.0], [1.57499, 0.125, -12.5, 0.0248, 0.9, 0.6, 0.3, 0.0, 100.0]],
    "s3": [[0.0, 3.0, 0.0, 1.0, 0.5, 0.8, 0.9, 1.0, 100.0]],
    "s4": [[-1.5338, 0.1, -10.0, 2.3068, 0.9, 0.6, 0.3, 0.0, 100.0], [2.17284, 0.125, -12.5, 0.39389, 0.9, 0.6, 0.3, 0.0, 100.0]],
    "s5": [[-0.01969, 0.1, -10.0, 1.25011, 0.9, 0.6, 0.3, 0.0, 100.0]],
    "s6": [[-1.13595, 0.57618, -10.0, 0.79363, 0.5, 0.8, 0.9, 1.0, 100.0], [-0.42484, -0.02487, -12.5, 0.24979, 0.7, 0.9, 0.4, 1.0, 100.0],
           [1.40964, 0.15, -15.0, 0.23892, 0.9, 0.6, 0.3, 0.0, 100.0], [2.20418, -0.0333, -17.5, 0.34716, 0.7, 0.9, 0.4, 1.0, 100.0]],
    "s7": [[-0.85863, 0.42857, -10.0, 0.54762, 0.5, 0.8, 0.9, 1.0, 100.0], [0.52133, 0.125, -12.5, 1.04541, 0.9, 0.6, 0.3, 0.0, 100.0],
           [0.0, 1000.0, 0.0, 990.0, 0.3, 0.3, 0.9, 0.0, 100.0]],
    "s9": [[-0.96928, 0.33508, -10.0, 0.3918, 0.5, 0.8, 0.9, 1.0, 100.0], [0.39016, 0.125, -12.5, 1.19393, 0.9, 0.6, 0.3, 0.0, 100.0]],
}


def fan_camera(w, pitch=0.004, rise=0.01, tilt=0.0):
    """eye at the origin, column c looks along (pitch (c - w / 2), rise + tilt, -1): one row.  The tilt is the basis' (the cameras of a
    batch share their screen)"""
    return np.array([1, 0, 0, 0, 1, 0, 0, -tilt, 1, 0, 0, 0, 1.0, pitch * w, 2 * rise], dtype=np.float64)


def rows_camera(w, h, pitch, rise, step):
    """... h rows, each `step` lower than the one above and all of them above the horizon: the basis' z axis carries the rise"""
    return np.array([1, 0, 0, 0, 1, 0, 0, -rise, 1, 0, 0, 0, 1.0, pitch * w, step * h], dtype=np.float64)


def down_camera():
    """every pixel looks straight down from the origin: a screen without extent"""
    return np.array([1, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1.0, 0.0, 0.0], dtype=np.float64)


class Case:
    def __init__(self, name, states, spheres, w, h, bounce_limit, camera, ground=DARK, cameras=None, what=""):
        self.name, self.states, self.w, self.h, self.bounce_limit, self.spp, self.what = name, states, w, h, bounce_limit, 1, what
        g = S.demo_ground().copy()
        g[9] = g[14] = ground
        self.scene = S.SceneData(np.array(SPHERES[spheres], dtype=np.float64), g, DIR_LIGHTS, POINT_LIGHTS, camera, T.sky("synth"))
        self.cameras = cameras  # a batch
        self.frames = 1 if cameras is None else len(cameras)
        self.units = self.frames * w * h * self.spp

    def __repr__(self):
        return self.name


CASES = {c.name: c for c in [
    Case("sky", (), "sky", 300, 1, 4, fan_camera(300), what="300 units that meet nothing: two waves, no task"),
    Case("s1", ("S1",), "s1", 64, 1, 4, fan_camera(64), what="64 dark hits from an empty ring"),
    Case("s2", ("S2", "S5"), "s2", 65, 1, 4, fan_camera(65), what="63 two-hit columns, one of sky, one dark"),
    Case("s3", ("S3",), "s3", 1, 1, 300, down_camera(), ground=MIRROR, what="one ray between a mirror ground and a mirror sphere above it, 300 bounces"),
    Case("s4", ("S4", "S8"), "s4", 200, 1, 4, fan_camera(200), what="120 dark columns, 16 of sky, 16 dark, 48 of sky"),
    Case("s5", ("S5",), "s5", 63, 1, 4, fan_camera(63), what="63 dark hits and a dead lane"),
    Case("s5_limit", ("S5",), "s5", 63, 1, 1, fan_camera(63), what="the same at a bounce limit of 1"),
    Case("s6", ("S6",), "s6", 88, 1, 2, fan_camera(88), what="32 two-hit columns, 8 mirror-then-sky, 24 of sky, 8 dark, 8 mirror-then-sky, 8 of sky; bounce limit 2"),
    Case("s7", ("S7",), "s7", 64, 1, 3, fan_camera(64), ground=MIRROR, what="22 columns of mirror, mirror ground and a dark sphere overhead, 42 dark; bounce limit 3"),
    Case("s9", ("S9",), "s9", 256, 16, 4, rows_camera(256, 16, 0.001, 0.01, 0.00001), what="16 rows of 256: 63 two-hit columns, one of sky, 192 dark"),
    Case("s10", ("S10",), "s2", 65, 1, 4, fan_camera(65), cameras=[fan_camera(65, tilt=t) for t in (0.0, 0.0002, -0.0002)], what="s2 from three cameras in one launch"),
]}


@functools.lru_cache(maxsize=None)
def sequences(name):
    """the oracle's account of every unit of the case (tests/support.py, oracle_hit_sequences), frames asserted finite"""
    c = CASES[name]
    q = T.oracle_hit_sequences(c.scene, c.w, c.h, c.bounce_limit, c.spp, c.cameras)
    assert q["paths"].size == c.units and all(np.isfinite(f).all() for f in q["frames"])
    return q


def launch_shape(units, block):
    """(workgroups, chunk) of an uncapped launch as plan_render lays it out: one queue word and whole chunks below 8 workgroups, a word
    per XCD and half chunks from 8 on"""
    grid = max(1, (units + block - 1) // block)
    return grid, CHUNK_SMALL if grid >= 1 << XCD_SHIFT else CHUNK


@functools.lru_cache(maxsize=None)
def decoupled(name, rules=M.RULES):
    """the model's waves of the decoupled launch of the case, in chunk order"""
    c, q = CASES[name], sequences(name)
    grid, chunk = launch_shape(c.units, COMPACT_BLOCK)
    return M.launch(M.decoupled_wave, c.units, chunk, grid * (COMPACT_BLOCK // 64), q["paths"], q["hits"], rules=rules)


@functools.lru_cache(maxsize=None)
def plain(name):
    c, q = CASES[name], sequences(name)
    grid, chunk = launch_shape(c.units, BLOCK)
    return M.launch(M.plain_wave, c.units, chunk, grid * (BLOCK // 64), q["paths"], q["hits"])


def total(waves, key):
    return sum(w[key] for w in waves)
