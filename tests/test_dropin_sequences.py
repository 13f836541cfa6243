"""A seeded model test of the DROP-IN layer (include/trt_hip.h section 1, csrc/trt_dropin.hip): project_scene, trt_render_frame,
render_frame, trt_render_frame_rgb8 and trt_render_frame_ansi are handed the scene with every call, and the default context behind
them keeps state from call to call -- a snapshot of the previous call's primitives, the two run counters of the moving / still
policy and whether the tables were built the cheap way, the skybox's face pointers, dimension and texel stamp, the eye tables, the
jitter table and the screen axes.  Generated sequences of scene edits, camera moves, policy changes, skybox calls, errors, trt_init and
trt_shutdown exercise that state against itself; every frame must be, bit for bit, the CPU oracle's for the scene the MODEL says is
current, and after every call trt_scene_is_moving(), the table builds and skybox uploads the call performed (trt_build_counts on the
borrowed default context, trt_hip_diag.h) and the patches of the tables it renders with must be the model's.

CHANGED, as csrc/trt_capi.hip (upload_primitives) decides it and the model repeats it: the spheres, either light array, or the
ground's point or normal differ BYTEWISE (counts included) from those of the previous call that got as far as comparing them.
Camera, ground materials, skybox, frame shape, bounce limit and samples per pixel do not count.  A call with a negative count or a
NULL array of a non-zero count is refused before the comparison and leaves everything as it was; a call whose cubemap is refused
(dimension 0, a NULL face) has compared -- and counted, and built -- already.

make_sequence(seed, steps) is pure (numpy only): plain-data operations, scripted motifs (one per transition of TRANSITIONS) woven into
random ones, drawn from a small per-seed pool of sphere counts, cameras and frame shapes.  Model follows a sequence without a GPU.
  * test_the_committed_sequences_cover_every_transition    (no GPU) every name in TRANSITIONS holds somewhere in the committed seeds
  * test_every_edit_is_visible_in_the_oracles_frames       (no GPU) the oracle's frame after every edit differs from the one before
  * test_the_model_agrees_with_a_stand_in_of_the_policy    (no GPU) moving / builds recomputed from the history alone
  * test_a_sequence_replayed_on_the_drop_in_entries        (gpu)    the replay; reproduce one seed with  -k "replayed and seed7"
Seeds with seed % 4 == 0 keep one sphere count and one cubemap dimension: a stale list or stale texels can then only give wrong
colours, never an index beyond the scene, which is what runs of deliberately broken builds need.

NOT pinned, on purpose: texels edited in place that the stamp does not sample and that the caller does not announce with
trt_invalidate_skybox() -- the header promises nothing about them (the model refuses to follow a sequence that renders in that state);
wall-clock cost of a build (the counts replace it); what a failed HIP call leaves behind."""
import ctypes as C
import os
import time
import zlib

import numpy as np
import pytest

from terminalraytracer_amd import scenes as S
from test_context_sequences import ARGUMENT, HIP

gpu = pytest.mark.gpu
SEEDS = tuple(range(12))
STEPS = 40
ENTRIES = ("project_scene", "trt_render_frame", "render_frame", "trt_render_frame_rgb8", "trt_render_frame_ansi")
PROJECT_SHOT = (20, 11, 10, 10)   # project_scene: the reference's fixed 10 bounces / 10 samples per pixel, on a 20 x 11 frame
DEFAULT_POLICY = (2, 3)
PATH_MIN, PATCHES_FROM, LIST_MAX, PATH_MAX = 12, 128, 256, 1024  # TRT_PATHGRID_MIN_SPHERES, TRT_PATCHES_FROM_SPHERES, TRT_LIST_MAX_SPHERES, TRT_PATH_MAX_SPHERES
BIG = 1500                        # the ("big", 1500, 5) scene of test_context_sequences: beyond LDS
THRESHOLDS = ((PATH_MIN - 1, PATH_MIN), (PATCHES_FROM - 1, PATCHES_FROM), (LIST_MAX, LIST_MAX + 1))
STAGE = tuple((x, y, z) for x in (-0.4, 0.0, 0.4) for y in (-0.4, 0.0, 0.4) for z in (-0.4, 0.0, 0.4) if (x, y, z) != (0.0, 0.0, 0.0))  # in front of every camera (orbit radius 1.99)
POINT_SPOTS = ((0.0, 0.0, 0.0), (3.0, 2.0, -3.0), (-3.0, 1.5, 3.0))
DIR_MASTER = np.array([[-1.0, -1.0, -1.0, 0.6, 0.6, 0.6], [0.6, -1.0, 0.2, 0.3, 0.2, 0.1], [-0.2, -1.0, 0.7, 0.1, 0.2, 0.3]])
POINT_MASTER = np.array([[0.0, 0.0, 0.0, 0.5, 0.5, 0.5, 10.0], [3.0, 2.0, -3.0, 0.4, 0.4, 0.2, 20.0]])
TILT = (0.28, 0.96, 0.0)
SKY_DIM = 32                      # 1024 texels a face: the stamp samples every fourth and the last of face 5
BAD = ("null_array", "negative_count", "dim0", "null_face")


# ---- the pool of a seed (plain data) ----

def make_pool(seed):
    rng = np.random.default_rng(5000 + seed)
    uniform = seed % 4 == 0
    n0 = int(rng.choice([24, 64, 150])) if uniform else int(rng.choice([40, 100, 200]))
    eyes = [int(i) for i in rng.choice(60, size=3, replace=False)]
    cams = [("anim", e, t) for e in eyes for t in (0, 1)]  # t = 1: the same eye, the orientation turned
    stored = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras_anim.npz"))["camera"]
    sizes = [(48, 27), (32, 18), (33, 17), (7, 5), (1, 1)]
    shots = [(w, h, int(rng.integers(1, 5)), int(rng.integers(1, 4))) for w, h in sizes]
    return {"seed": seed, "uniform": uniform, "n0": n0, "cams": cams, "shots": shots, "master_seed": 31 + seed,
            "eyes": [tuple(float(v) for v in stored[e, 9:12]) for e in eyes],  # where the generator puts a sphere, no other hides it from these
            "sky_dims": (SKY_DIM,) if uniform else (SKY_DIM, 1, 5, 64)}


def master_spheres(pool, n):
    """the first n spheres of the seed's scene; the spheres that cross a threshold one at a time stand in front of every camera"""
    sph = S.synth_spheres(BIG, 5) if n == BIG else S.synth_spheres(max(n, 1), pool["master_seed"])[:n]
    for i, c in ((PATH_MIN - 1, (0.5, 0.3, 0.0)), (PATCHES_FROM - 1, (-0.5, 0.2, 0.3)), (LIST_MAX, (0.0, -0.4, -0.5))):
        if i < n != BIG:
            sph[i, :4] = (*c, 0.4)
    for eye in pool["eyes"]:  # no eye inside a sphere or close behind one: such spheres stand behind the cameras instead
        sph[np.linalg.norm(sph[:, :3] - np.array(eye), axis=1) < sph[:, 3] + 0.5, 2] += 3.0
    return sph


def stamp_of(sky):
    """skybox_stamp of csrc/trt_capi.hip: FNV-1a over 256 texels a face at a fixed stride, then the last texel of face 5"""
    mask, h = (1 << 64) - 1, 1469598103934665603
    dim = sky.shape[1]
    face = dim * dim
    step = face // 256 or 1
    flat = sky.reshape(6, face, 3)
    for f in range(6):
        for byte in flat[f, ::step].reshape(-1).tolist():
            h = ((h ^ byte) * 1099511628211) & mask
    r, g, b = (int(v) for v in flat[5, face - 1])
    return ((h ^ (r << 16 | g << 8 | b)) * 1099511628211) & mask


def unsampled(sky):
    """boolean [6, dim * dim]: the texels skybox_stamp does not read"""
    face = sky.shape[1] ** 2
    m = np.ones((6, face), dtype=bool)
    m[:, ::face // 256 or 1] = False
    m[5, face - 1] = False
    return m


# ---- the model ----

class Model:
    """What the drop-in layer must do with a sequence: the caller's scene (numpy arrays, edited in place where the operation says
    so), the default context's state, and one record per operation for the transition predicates."""

    def __init__(self, pool):
        self.pool = pool
        self.spheres = master_spheres(pool, pool["n0"])
        self.ground = S.demo_ground()
        self.dir, self.point = DIR_MASTER[:1].copy(), POINT_MASTER[:1].copy()
        self.skies = [S.synth_sky(SKY_DIM, seed=pool["seed"] + 1)]  # every cubemap a caller ever held stays alive: pointers are never reused
        self.sky = 0
        self.policy = DEFAULT_POLICY   # global to the library: survives trt_shutdown
        self.ctx = None                # the default context's state
        self.pending, self.sky_pending = [], []
        self.last_render = None
        self.records = []
        self.total = [0, 0]

    # -- what the caller holds --
    def snapshot(self):
        return {"spheres": self.spheres.copy(), "ground": self.ground.copy(), "dir": self.dir.copy(), "point": self.point.copy(),
                "sky": self.skies[self.sky].copy()}

    def primitives(self):
        return (self.spheres.tobytes(), self.dir.tobytes(), self.point.tobytes(), self.ground[:6].tobytes())

    def sky_key(self):
        return zlib.crc32(self.skies[self.sky].tobytes()), self.skies[self.sky].shape[1]

    # -- the default context --
    def _fresh(self):
        self.ctx = {"changes": 0, "still": 0, "moving": False, "built": False, "built_moving": False, "prims": None,
                    "sky_buf": None, "sky_dim": -1, "sky_stamp": None, "sky_content": None, "builds": 0, "uploads": 0}

    def _upload_sky(self, rec):
        c, sky = self.ctx, self.skies[self.sky]
        c.update(sky_buf=self.sky, sky_dim=sky.shape[1], sky_stamp=stamp_of(sky), sky_content=self.sky_key())
        c["uploads"] += 1
        rec["uploads"] += 1

    def patches(self):
        c = self.ctx
        if c is None or not c["built"]:
            return None
        n = len(c["prims"][0]) // 72
        if n < PATH_MIN or n > PATH_MAX:
            return (0, 0)
        m = 0 if c["built_moving"] or n < PATCHES_FROM else 2
        return (m, 6 * m * m if m else 1)

    def apply(self, op):
        kind = op[0]
        rec = {"op": op, "kind": kind, "code": 0, "ctx_before": self.ctx is not None, "was_moving": bool(self.ctx and self.ctx["moving"]),
               "changed": None, "builds": 0, "uploads": 0, "policy": self.policy, "edits": [], "sky_edits": []}
        if kind in ("render", "bad"):
            self._call(rec)
        elif kind == "policy":
            if op[1] < 0 or op[2] < 1:
                rec["code"] = ARGUMENT
            else:
                self.policy = (op[1], op[2])
                if op[1] == 0 and self.ctx:
                    self.ctx["moving"] = False  # "never": a scene that counts as moving stops doing so at once
        elif kind == "shutdown":
            self.ctx = None
        elif kind == "init":
            if self.ctx is None:
                self._fresh()
        elif kind == "upload_skybox":
            if op[1] == "null":
                rec["code"] = ARGUMENT  # refused before a context is made
            else:
                if self.ctx is None:
                    self._fresh()
                self._upload_sky(rec)
        elif kind == "invalidate":
            if self.ctx:
                self.ctx["sky_dim"] = -1
            self.sky_pending.append("invalidate")
        elif kind in ("sky_new", "sky_edit"):
            rec["before"] = self.snapshot()
            self._sky(op)
            rec["after"] = self.snapshot()
            self.sky_pending.append(":".join(str(x) for x in op))
        else:
            rec["before"] = self.snapshot()
            self._edit(op)
            rec["after"] = self.snapshot()
            self.pending.append(kind)
        rec.update(policy_after=self.policy, ctx_after=self.ctx is not None, moving=bool(self.ctx and self.ctx["moving"]), patches=self.patches(),
                   n=len(self.spheres), nd=len(self.dir), np=len(self.point),
                   run=(self.ctx["changes"], self.ctx["still"]) if self.ctx else None)
        self.total = [self.ctx["builds"], self.ctx["uploads"]] if self.ctx else [0, 0]
        rec["total"] = tuple(self.total)
        self.records.append(rec)
        return rec

    def _call(self, rec):
        """one drop-in entry, as refresh_default_scene and upload_primitives go through it"""
        op = rec["op"]
        bad = op[1] if op[0] == "bad" else None
        entry, cam, shot = op[2:5] if bad else op[1:4]
        rec.update(entry=entry, cam=cam, shot=shot, bad=bad)
        assert entry != "project_scene" or (shot == PROJECT_SHOT and not bad), "project_scene has fixed limits and aborts on an error"
        if self.ctx is None:
            self._fresh()
        c = self.ctx
        if bad in ("null_array", "negative_count"):
            assert bad != "null_array" or len(self.spheres), "a NULL array needs a non-zero count"
            rec["code"] = ARGUMENT
            return
        prims = self.primitives()
        rec["changed"] = changed = prims != c["prims"]
        rec["first"] = c["prims"] is None
        rec["n_before"] = None if c["prims"] is None else tuple(len(c["prims"][k]) // s for k, s in ((0, 72), (1, 48), (2, 56)))
        rec["edits"], self.pending = self.pending, []
        c["prims"] = prims
        moving_after, still_after = self.policy
        if changed:
            c["still"] = 0
            c["changes"] += 1
            if c["changes"] >= moving_after > 0:
                c["moving"] = True
        else:
            c["changes"] = 0
            c["still"] += 1
            if c["still"] >= still_after:
                c["moving"] = False
        if not c["built"] or changed or c["built_moving"] != c["moving"]:
            c["built"], c["built_moving"] = True, c["moving"]
            c["builds"] += 1
            rec["builds"] += 1
        if bad:  # dim0, null_face: refused where the cubemap would be uploaded; what the context holds of the old one stays
            rec["code"] = ARGUMENT
            return
        sky = self.skies[self.sky]
        if not (c["sky_dim"] == sky.shape[1] and c["sky_buf"] == self.sky and c["sky_stamp"] == stamp_of(sky)):
            self._upload_sky(rec)
        assert c["sky_content"] == self.sky_key(), "texels edited in place outside the stamp and not announced: the header promises nothing"
        rec["sky_edits"], self.sky_pending = self.sky_pending, []
        rec["frame"] = self.snapshot()
        rec["previous_render"] = self.last_render
        self.last_render = len(self.records)

    def _edit(self, op):
        kind = op[0]
        if kind == "move":     # a sphere to a place in front of the cameras, several radii from where it was
            i, to = op[1], np.array(op[2])
            assert np.linalg.norm(to - self.spheres[i, :3]) >= 3 * self.spheres[i, 3], "a far move is several radii long"
            self.spheres[i, :3] = to
        elif kind == "swap":   # two distant spheres change places
            i, j = op[1], op[2]
            assert np.linalg.norm(self.spheres[i, :3] - self.spheres[j, :3]) >= 3 * max(self.spheres[i, 3], self.spheres[j, 3])
            self.spheres[[i, j], :3] = self.spheres[[j, i], :3]
        elif kind == "radius":
            self.spheres[op[1], 3] *= 3.0
        elif kind == "material":
            self.spheres[op[1], 4:7] = 1.0 - self.spheres[op[1], 4:7]
        elif kind == "count":
            self.spheres = master_spheres(self.pool, op[1])
        elif kind == "dir_turn":
            d = self.dir[op[1], :3].copy()
            new = np.array([-(d[0] + np.copysign(1.0, d[0])), d[1], -(d[2] + np.copysign(1.0, d[2]))])
            assert np.dot(d, new) / (np.linalg.norm(d) * np.linalg.norm(new)) < 0.5, "a turn by more than 60 degrees"
            self.dir[op[1], :3] = new
        elif kind == "point_move":
            self.point[op[1], :3] = op[2]
        elif kind == "light_colour":
            lights = self.dir if op[1] == "dir" else self.point
            lights[op[2], 3:6] = 1.0 - 0.75 * lights[op[2], 3:6][::-1]
        elif kind == "dir_count":
            self.dir = DIR_MASTER[:op[1]].copy()
        elif kind == "point_count":
            self.point = POINT_MASTER[:op[1]].copy()
        elif kind == "ground_raise":
            self.ground[1] += op[1]
        elif kind == "ground_tilt":
            self.ground[3:6] = (0.0, 1.0, 0.0) if tuple(self.ground[3:6]) == TILT else TILT
        elif kind == "ground_material":  # reflectivity 0 <-> 0.6 and the two colours exchanged
            refl = 0.6 if self.ground[9] != 0.6 else 0.0
            even, odd = self.ground[6:9].copy(), self.ground[11:14].copy()
            self.ground[6:9], self.ground[11:14], self.ground[9], self.ground[14] = odd, even, refl, refl
        else:
            raise AssertionError(kind)

    def _sky(self, op):
        sky = self.skies[self.sky]
        if op[0] == "sky_new":
            if op[1] == "same":      # new face pointers, the same texels
                new = sky.copy()
            elif op[1] == "invert":  # new pointers, every texel another, the same dimension
                new = 255 - sky
            else:                    # another dimension
                new = S.synth_sky(op[2], seed=100 + len(self.skies))
            self.skies.append(np.ascontiguousarray(new))
            self.sky = len(self.skies) - 1
            return
        assert sky.shape[1] ** 2 >= 512, "in-place edits need a cubemap with texels the stamp does not sample"
        flat = sky.reshape(6, -1, 3)
        off = unsampled(sky)
        flat[off] = 255 - flat[off]  # three quarters of the image, none of it in the stamp: visible, and unnoticed by itself
        if op[1] == "texel0":
            flat[0, 0] = 255 - flat[0, 0]
        elif op[1] == "last":
            flat[5, -1] = 255 - flat[5, -1]
        else:
            assert op[1] == "unsampled"


# ---- the transitions: predicates over (records before, this record) ----

def _good(r):
    return r["kind"] == "render" and r["code"] == 0


def _called(r):
    """the call reached the comparison of the primitives"""
    return r["kind"] in ("render", "bad") and r["changed"] is not None


def _previous(hist, test):
    for r in reversed(hist):
        if test(r):
            return r
    return None


def _only(tag, changed=True):
    def t(hist, rec):
        return _good(rec) and rec["edits"] == [tag] and rec["changed"] is changed and not rec["first"] and rec["builds"] == (1 if changed else 0)
    t.__doc__ = f"a call after nothing but one `{tag}` edit: {'a change, one build' if changed else 'not a change, no build'}"
    return t


def _moves(hist, rec):
    """a far move (or two distant spheres exchanged) at constant count"""
    return (_good(rec) and rec["changed"] and not rec["first"] and rec["edits"] and set(rec["edits"]) <= {"move", "swap"}
            and rec["n_before"][0] == rec["n"] and rec["builds"] == 1)


def _count(a, b, which=0):
    def t(hist, rec):
        return _good(rec) and not rec["first"] and rec["n_before"][which] == a and (rec["n"], rec["nd"], rec["np"])[which] == b and rec["builds"] == 1
    t.__doc__ = f"{('sphere', 'directional light', 'point light')[which]} count {a} -> {b} between two calls"
    return t


def _still_patches(hist, rec):
    """a scene of 128 spheres or more, promoted after it has moved: the automatic patches (2, 24) where the call before had none"""
    p = _previous(hist, _called)
    return _good(rec) and rec["patches"] == (2, 24) and p is not None and p["patches"] == (0, 1) and not rec["changed"]


def _no_light(hist, rec):
    """a frame of a scene without any light"""
    return _good(rec) and rec["nd"] == 0 and rec["np"] == 0


def _camera_only(what):
    def t(hist, rec):
        if not (_good(rec) and rec["changed"] is False and rec["builds"] == 0 and rec["uploads"] == 0 and not rec["edits"] and not rec["sky_edits"]
                and hist and _good(hist[-1]) and rec["entry"] == hist[-1]["entry"]):
            return False
        p = hist[-1]
        (w, h, b, spp), (pw, ph, pb, pspp), same_cam = rec["shot"], p["shot"], rec["cam"] == p["cam"]
        rest = {"size": (b, spp) == (pb, pspp) and same_cam, "spp": (w, h, b) == (pw, ph, pb) and same_cam, "bounces": (w, h, spp) == (pw, ph, pspp) and same_cam}
        return {"eye": rec["cam"][1] != p["cam"][1] and rec["shot"] == p["shot"],
                "orientation": rec["cam"][1] == p["cam"][1] and rec["cam"][2] != p["cam"][2] and rec["shot"] == p["shot"],
                "size": (w, h) != (pw, ph) and rest["size"], "spp": spp != pspp and rest["spp"], "spp_1": spp == 1 != pspp and rest["spp"],
                "spp_64": spp == 64 != pspp and rest["spp"], "bounces": b != pb and rest["bounces"]}[what]
    t.__doc__ = f"nothing but the camera / frame shape differs from the call before ({what}): no change, no build, no upload"
    return t


def _sky(tag, uploads=1, dim=None):
    def t(hist, rec):
        return (_good(rec) and not rec["first"] and rec["sky_edits"] == [tag] and rec["uploads"] == uploads and rec["builds"] == 0
                and (dim is None or dim(rec["frame"]["sky"].shape[1])))
    t.__doc__ = f"a call after `{tag}`: {uploads} upload(s), no table build"
    return t


def _sky_invalidated(hist, rec):
    """texels the stamp does not sample edited in place, then trt_invalidate_skybox(): one upload"""
    return _good(rec) and rec["sky_edits"] == ["sky_edit:unsampled", "invalidate"] and rec["uploads"] == 1


def _upload_first(hist, rec):
    """trt_upload_skybox ahead of the first frame of a context; the frame uploads nothing"""
    p = hist[-1] if hist else None
    return _good(rec) and rec["first"] and rec["uploads"] == 0 and p is not None and p["kind"] == "upload_skybox" and p["code"] == 0 and not p["ctx_before"]


def _upload_between(hist, rec):
    """trt_upload_skybox of ANOTHER cubemap between two frames; the frame after it uploads nothing and shows it"""
    p = hist[-1] if hist else None
    return (_good(rec) and not rec["first"] and rec["uploads"] == 0 and p is not None and p["kind"] == "upload_skybox" and p["code"] == 0
            and len(hist) > 1 and hist[-2]["kind"] == "sky_new")


def _moving_exactly(hist, rec):
    """moving exactly at the moving_after-th consecutive change (moving_after >= 2)"""
    return _called(rec) and rec["moving"] and not rec["was_moving"] and rec["policy"][0] >= 2 and rec["run"][0] == rec["policy"][0]


def _interrupted(hist, rec):
    """change, unchanged, change: the run is interrupted and does not reach moving_after = 2"""
    calls = [r for r in hist if _called(r)][-2:]
    return (_called(rec) and rec["changed"] and not rec["moving"] and rec["policy"][0] == 2 and len(calls) == 2 and calls[0]["changed"]
            and not calls[0]["first"] and not calls[1]["changed"] and rec["run"][0] == 1)


def _promotion(hist, rec):
    """promotion exactly at the still_after-th unchanged call: one build, no primitive change"""
    return _good(rec) and rec["was_moving"] and not rec["moving"] and rec["changed"] is False and rec["run"][1] == rec["policy"][1] >= 2 and rec["builds"] == 1


def _policy_1_1(hist, rec):
    """(1, 1): moving at the first change, promoted at the first unchanged call"""
    p = _previous(hist, _called)
    return (_good(rec) and rec["policy"] == (1, 1) and rec["changed"] is False and rec["builds"] == 1 and not rec["moving"]
            and p is not None and p["policy"] == (1, 1) and p["changed"] and p["moving"] and not p["was_moving"])


def _policy_0_start(hist, rec):
    """(0, k) from a context's first call on: the third change in a row still builds the full tables"""
    calls = [r for r in hist if _called(r)]
    k = max([i for i, r in enumerate(calls) if r["first"]], default=None)
    return (_good(rec) and rec["policy"][0] == 0 and rec["changed"] and k is not None and len(calls) - k >= 2
            and all(r["policy"][0] == 0 and r["changed"] for r in calls[k:]) and not rec["moving"])


def _policy_0_moving(hist, rec):
    """(0, k) set while the scene is moving: not moving at once, and the next change builds the full tables"""
    p = _previous(hist, lambda r: "before" not in r)  # the edit itself lies between the two
    return (_good(rec) and rec["changed"] and not rec["moving"] and rec["builds"] == 1 and p is not None and p["kind"] == "policy" and p["code"] == 0
            and p["op"][1] == 0 and p["was_moving"] and not p["moving"])


def _policy_invalid(hist, rec):
    """invalid arguments are refused and change nothing"""
    return rec["kind"] == "policy" and rec["code"] == ARGUMENT and rec["policy"] == rec["policy_after"]


def _all_entries(hist, rec):
    """all five entries within one run of consecutive changes"""
    seen = set()
    for r in reversed(hist + [rec]):
        if "before" in r:  # an edit
            continue
        if not (_good(r) and r["changed"]):
            break
        seen.add(r["entry"])
    return _good(rec) and seen == set(ENTRIES)


def _shutdown_moving(hist, rec):
    """trt_shutdown while the scene is moving: trt_scene_is_moving() is 0"""
    return rec["kind"] == "shutdown" and rec["was_moving"] and not rec["moving"]


def _fresh_after_shutdown(hist, rec):
    """the call after trt_shutdown builds everything on a fresh context, unchanged scene or not"""
    return (_good(rec) and rec["first"] and rec["builds"] == 1 and rec["uploads"] == 1 and not rec["edits"]
            and any(r["kind"] == "shutdown" and r["ctx_before"] for r in hist))


def _init_live(hist, rec):
    """trt_init(0) on a live context changes nothing"""
    return rec["kind"] == "init" and rec["ctx_before"]


def _error(bad):
    def t(hist, rec):
        p = _previous(hist, lambda r: r["kind"] in ("render", "bad"))
        return rec["kind"] == "bad" and rec["bad"] == bad and rec["code"] == ARGUMENT and p is not None and _good(p)
    t.__doc__ = f"an error after a good call: {bad}"
    return t


def _after_error(edited, late):
    def t(hist, rec):
        p = _previous(hist, lambda r: r["kind"] in ("render", "bad"))
        return (_good(rec) and p is not None and p["kind"] == "bad" and (p["changed"] is not None) == late
                and bool(rec["edits"] or (late and p["edits"])) == edited)
    t.__doc__ = (f"a good call after an error refused {'at the cubemap (the primitives were compared)' if late else 'before the comparison'}, "
                 f"the scene {'edited' if edited else 'unchanged'} since the last good call")
    return t


TRANSITIONS = {"far_move_at_constant_count": _moves, "material_only": _only("material"), "radius_only": _only("radius"),
               "patches_once_still": _still_patches, "no_light_at_all": _no_light,
               "light_direction_only": _only("dir_turn"), "light_position_only": _only("point_move"), "light_colour_only": _only("light_colour"),
               "ground_point": _only("ground_raise"), "ground_normal": _only("ground_tilt"), "ground_materials_only": _only("ground_material", changed=False),
               "sky_new_pointers_same_texels": _sky("sky_new:same"), "sky_new_pointers_other_texels": _sky("sky_new:invert"),
               "sky_dim_1": _sky("sky_new:dim:1"), "sky_dim_not_a_power_of_two": _sky("sky_new:dim:5"), "sky_larger_dim": _sky("sky_new:dim:64"),
               "sky_texel_0_of_face_0_in_place": _sky("sky_edit:texel0"), "sky_last_texel_of_face_5_in_place": _sky("sky_edit:last"),
               "sky_unsampled_then_invalidate": _sky_invalidated, "upload_skybox_before_first_frame": _upload_first,
               "upload_skybox_between_frames": _upload_between,
               "moving_exactly_at_moving_after": _moving_exactly, "interrupted_run_does_not_reach": _interrupted,
               "promotion_exactly_at_still_after": _promotion, "policy_1_1": _policy_1_1, "policy_0_from_the_start": _policy_0_start,
               "policy_0_set_while_moving": _policy_0_moving, "invalid_policy_refused": _policy_invalid,
               "all_five_entries_in_one_run_of_changes": _all_entries,
               "shutdown_while_moving": _shutdown_moving, "fresh_context_after_shutdown": _fresh_after_shutdown, "init_on_a_live_context": _init_live}
for _a, _b in THRESHOLDS + ((200, BIG), (0, 40)):
    TRANSITIONS[f"spheres_{_a}_to_{_b}"], TRANSITIONS[f"spheres_{_b}_to_{_a}"] = _count(_a, _b), _count(_b, _a)
for _a, _b in ((0, 1), (1, 3)):
    TRANSITIONS[f"directional_{_a}_to_{_b}"], TRANSITIONS[f"directional_{_b}_to_{_a}"] = _count(_a, _b, 1), _count(_b, _a, 1)
TRANSITIONS.update({"point_0_to_2": _count(0, 2, 2), "point_2_to_0": _count(2, 0, 2)})
TRANSITIONS.update({f"camera_only_{w}": _camera_only(w) for w in ("eye", "orientation", "size", "spp", "spp_1", "spp_64", "bounces")})
TRANSITIONS.update({f"error_{bad}": _error(bad) for bad in BAD})
TRANSITIONS.update({f"good_after_{'late' if late else 'early'}_error_{'edited' if e else 'unchanged'}": _after_error(e, late) for e in (False, True) for late in (False, True)})
UNIFORM_TRANSITIONS = ("far_move_at_constant_count", "material_only", "radius_only", "light_direction_only", "ground_point", "sky_new_pointers_other_texels",
                       "sky_texel_0_of_face_0_in_place", "sky_last_texel_of_face_5_in_place", "policy_0_set_while_moving", "promotion_exactly_at_still_after")


def transitions_of(records):
    return {name for k, rec in enumerate(records) for name, test in TRANSITIONS.items() if test(records[:k], rec)}


# ---- the generator ----

def make_sequence(seed, steps=STEPS):
    """At least `steps` plain-data operations for the pool of `seed`; deterministic; no GPU."""
    pool = make_pool(seed)
    rng = np.random.default_rng(6000 + seed)
    model = Model(pool)
    ops = []
    cams, shots, uniform = pool["cams"], pool["shots"], pool["uniform"]
    state = {"cam": cams[0], "shot": shots[0], "tripled": set(), "staged": None}

    def emit(*op):
        ops.append(op)
        return model.apply(op)

    pick = lambda seq: seq[int(rng.integers(len(seq)))]

    def render(entry=None, cam=None, shot=None):
        entry = entry or pick(ENTRIES[1:])
        state["cam"], state["shot"] = cam or state["cam"], shot or state["shot"]
        return emit("render", entry, state["cam"], PROJECT_SHOT if entry == "project_scene" else state["shot"])

    def look(small=False):
        """another camera and shape for what follows; frames of the large scenes stay small"""
        state["cam"] = pick(cams)
        state["shot"] = pick(shots[1:3] if small or len(model.spheres) > 300 else shots[:3])

    def policy(*p):
        if model.policy != p:
            emit("policy", *p)

    def n():
        return len(model.spheres)

    def in_sight(i, place):
        """no other sphere lies between `place`, where sphere i is to stand, and any eye of the pool"""
        others = np.delete(model.spheres, i, axis=0)
        for eye in pool["eyes"]:
            d = np.array(place) - np.array(eye)
            length = float(np.linalg.norm(d))
            oc = others[:, :3] - np.array(eye)
            t = np.clip(oc @ (d / length), 0.0, length)
            if (np.linalg.norm(oc - t[:, None] * (d / length), axis=1) < others[:, 3]).any():
                return False
        return True

    def movable(small=False):
        """(sphere, the place of the stage farthest from it that every eye sees) of a random sphere that has not been tripled; the sphere
        is the one a later material or radius edit takes"""
        lo, hi = (0.2, 0.3) if small else (0.25, 0.5)
        i = pick([i for i in range(n()) if i not in state["tripled"] and lo <= model.spheres[i, 3] <= hi])
        places = sorted(STAGE, key=lambda s: -float(np.linalg.norm(np.array(s) - model.spheres[i, :3])))
        places = [s for s in places if np.linalg.norm(np.array(s) - model.spheres[i, :3]) >= 3 * model.spheres[i, 3]]
        to = next((s for s in places if in_sight(i, s)), places[0])
        state["staged"] = i
        return i, to

    def staged():
        """the sphere on the stage (one is put there first if none is)"""
        if state["staged"] is None:
            emit("move", *movable())
            render()
        return state["staged"]

    def spheres(k):
        if n() != k:
            emit("count", k)
            state["tripled"], state["staged"] = set(), None

    def some_spheres():
        if n() < 20 or n() > 300:
            spheres(pool["n0"])

    def change():
        """one visible change of the primitives"""
        some_spheres()
        what = pick(["move", "move", "swap", "material", "dir_turn", "ground_raise"])
        if what == "move":
            emit("move", *movable())
        elif what == "swap":
            swap()
        elif what == "material":
            emit("material", staged())
        elif what == "dir_turn" and len(model.dir):
            emit("dir_turn", int(rng.integers(len(model.dir))))
        else:
            emit("ground_raise", 0.5 if model.ground[1] < -2.0 else -0.5)

    def settle():
        """unchanged calls until the context is still, its run of changes over"""
        render()
        while model.ctx["moving"]:
            render()

    def get_moving():
        policy(2, 3)
        while not (model.ctx and model.ctx["moving"]):
            change()
            render()

    # -- the motifs --
    def m_moves():
        some_spheres(), look()
        render()
        for _ in range(3):
            emit("move", *movable()) if rng.random() < 0.6 else swap()
            render()

    def swap():
        """the sphere on the stage changes places with the one farthest from it"""
        i = staged()
        j = int(max((j for j in range(n()) if j not in state["tripled"] and j != i), key=lambda j: float(np.linalg.norm(model.spheres[j, :3] - model.spheres[i, :3]))))
        emit("swap", i, j)
        state["staged"] = j

    def m_material_radius():
        some_spheres(), look()
        i, to = movable(small=True)
        emit("move", i, to)  # within 0.7 of the origin: tripled, it still ends short of every camera
        render()
        emit("material", i)
        render()
        emit("radius", i)
        state["tripled"].add(i)
        state["staged"] = None
        render()

    def m_threshold(which=None):
        a, b = THRESHOLDS[int(rng.integers(len(THRESHOLDS))) if which is None else which % len(THRESHOLDS)]
        look(small=True)
        policy(2, 2)
        spheres(a), render()
        spheres(b), render()
        spheres(a), render()
        spheres(b), render()   # moving by now: no patches at 128 ...
        settle()               # ... until the scene is still

    def m_big():
        look(small=True)
        spheres(200), render()
        spheres(BIG), render()
        render(cam=pick(cams))
        spheres(200), render()

    def m_zero():
        look()
        spheres(40), render()
        spheres(0), render()
        render(cam=pick(cams))
        spheres(40), render()

    def m_lights():
        some_spheres(), look()
        if not len(model.dir):
            emit("dir_count", 1)
        if not len(model.point):
            emit("point_count", 2)
        render()
        emit("dir_turn", int(rng.integers(len(model.dir)))), render()
        k = int(rng.integers(len(model.point)))
        emit("point_move", k, max(POINT_SPOTS, key=lambda s: float(np.linalg.norm(np.array(s) - model.point[k, :3])))), render()
        emit("light_colour", "dir", 0) if rng.random() < 0.5 else emit("light_colour", "point", k)
        render()

    def m_light_counts():
        some_spheres(), look()
        emit("dir_count", 1), emit("point_count", 2), render()
        emit("dir_count", 3), render()
        emit("point_count", 0), render()
        emit("dir_count", 1), render()
        emit("dir_count", 0), render()      # no light at all
        emit("point_count", 2), render()
        emit("dir_count", 1), render()

    def m_ground():
        some_spheres(), look()
        settle()
        emit("ground_material"), render()
        emit("ground_tilt"), render()
        emit("ground_raise", 0.7 if model.ground[1] < -1.9 else -0.7), render()
        emit("ground_material"), render()

    def m_camera():
        some_spheres()
        entry = pick(ENTRIES[1:])
        eye = pick(cams)
        w, h, b, spp = pick(shots[:3])
        spp = 2 if spp == 1 else spp
        settle()
        render(entry, eye, (w, h, b, spp))
        render(entry, (eye[0], eye[1], 1 - eye[2]))                                           # the orientation turned
        render(entry, pick([c for c in cams if c[1] != eye[1]]))                              # the eye moved
        render(entry, shot=pick([(x, y, b, spp) for x, y, _, _ in shots if (x, y) != (w, h)]))  # another size
        w, h = state["shot"][:2]
        render(entry, shot=(w, h, b % 4 + 1, spp))                                            # another bounce limit
        b = state["shot"][2]
        render(entry, shot=(w, h, b, 1))
        render(entry, shot=(7, 5, b, 1))
        render(entry, shot=(7, 5, b, 64))
        render(entry, shot=(7, 5, b, 3))
        state["shot"] = shots[0]

    def base_sky():
        if model.skies[model.sky].shape[1] != SKY_DIM:
            emit("sky_new", "dim", SKY_DIM)

    def m_sky_pointers():
        some_spheres(), look()
        settle()
        emit("sky_new", "same"), render()
        emit("sky_new", "invert"), render()
        if not uniform:
            for dim in rng.permutation(pool["sky_dims"][1:]).tolist():
                emit("sky_new", "dim", int(dim)), render()
            render(cam=pick(cams))
            base_sky(), render()

    def m_sky_in_place():
        some_spheres(), look()
        base_sky(), settle()
        for what in rng.permutation(["texel0", "last", "unsampled"]).tolist():
            emit("sky_edit", what)
            if what == "unsampled":
                emit("invalidate")
            render()

    def m_upload():
        some_spheres(), look()
        settle()
        emit("sky_new", "invert")
        emit("upload_skybox", "current")
        render()
        emit("upload_skybox", "null")
        render()

    def m_policy_moving():
        some_spheres(), look()
        ma, sa = int(pick([2, 3])), int(pick([2, 3]))
        policy(ma, sa)
        settle()
        for _ in range(ma + 1):
            change(), render()
        for _ in range(sa + 1):
            render(cam=pick(cams))

    def m_interrupted():
        some_spheres(), look()
        policy(2, 3)
        settle()
        change(), render()
        render()
        change(), render()
        render()
        change(), render()

    def m_policy_1_1():
        some_spheres(), look()
        policy(1, 1)
        settle()
        change(), render()
        render()
        change(), render()
        render()
        policy(*DEFAULT_POLICY)

    def m_policy_0_start():
        look()
        emit("shutdown")
        policy(0, int(pick([1, 3])))
        some_spheres()
        render()
        for _ in range(3):
            change(), render()
        policy(*DEFAULT_POLICY)

    def m_policy_0_moving():
        some_spheres(), look()
        get_moving()
        emit("policy", 0, int(pick([2, 3])))
        change(), render()
        change(), render()
        render()
        policy(*DEFAULT_POLICY)

    def m_policy_invalid():
        emit("policy", *pick([(-1, 3), (2, 0), (0, 0), (-2, -2)]))
        render()

    def m_entries():
        some_spheres(), look(small=True)
        policy(2, 3)
        render()
        for entry in rng.permutation(list(ENTRIES)).tolist():
            change(), render(entry)
        settle()

    def m_lifetime():
        some_spheres(), look()
        get_moving()
        emit("shutdown")
        render()
        emit("init")
        render()
        change(), render()

    def m_errors():
        some_spheres(), look()
        render()
        for edited in rng.permutation([0, 1]).tolist():
            emit("bad", pick(BAD), pick(ENTRIES[1:]), state["cam"], state["shot"])
            if edited:
                change()
            render()
            render()

    def m_errors_each():
        some_spheres(), look(small=True)
        for bad in rng.permutation(list(BAD)).tolist():
            render()
            change() if rng.random() < 0.5 else None
            emit("bad", bad, pick(ENTRIES[1:]), state["cam"], state["shot"])
        render()

    def m_upload_first():
        emit("shutdown")
        emit("upload_skybox", "current")
        look()
        render()

    def filler():
        kind = pick(["render"] * 4 + ["change"] * 4 + ["camera"] * 2 + ["policy", "sky"])
        if kind == "render":
            render()
        elif kind == "change":
            change(), render()
        elif kind == "camera":
            look(), render()
        elif kind == "policy":
            policy(*pick([(2, 3), (1, 2), (3, 2), (0, 3)]))
        else:
            emit("sky_new", pick(["same", "invert"])), render()

    anywhere = [m_moves, m_material_radius, m_lights, m_light_counts, m_ground, m_camera, m_sky_pointers, m_sky_in_place, m_upload, m_policy_moving,
                m_interrupted, m_policy_1_1, m_policy_0_start, m_policy_0_moving, m_policy_invalid, m_entries, m_lifetime, m_errors, m_errors_each,
                m_upload_first]
    counting = [m_threshold, m_zero]
    motifs = anywhere if uniform else anywhere + counting
    if seed % 3 == 1:
        emit("upload_skybox", "current")  # ahead of the first frame
    render(shot=shots[0])
    for i in range(2):  # every motif opens some seed's sequence, whatever the draws below
        anywhere[(seed * 2 + i) % len(anywhere)]()
    if uniform:  # what a deliberately broken build is run against: stale lists, stale texels, stale policy
        for m in {0: (m_sky_in_place, m_moves), 4: (m_policy_0_moving, m_material_radius, m_lights), 8: (m_sky_pointers, m_ground)}.get(seed, ()):
            m()
    else:
        (m_zero, m_big, m_threshold)[seed % 4 - 1]() if seed % 4 != 3 else m_threshold(seed // 4 + 1)
        m_threshold(seed // 4)
    while len(ops) < steps:
        if rng.random() < 0.5:
            pick(motifs)()
        else:
            filler()
    policy(*DEFAULT_POLICY)
    return ops


def run_model(seed):
    model = Model(make_pool(seed))
    for op in make_sequence(seed):
        model.apply(op)
    return model


# ---- without a GPU ----

def test_the_generator_is_deterministic_and_long_enough():
    assert len(SEEDS) == 12
    for seed in SEEDS:
        first, again = make_sequence(seed), make_sequence(seed)
        assert first == again, seed
        assert STEPS <= len(first) <= 2 * STEPS, (seed, len(first))
        for op in first:
            if op[0] == "render":
                w, h, b, spp = op[3]
                assert op[3] == PROJECT_SHOT if op[1] == "project_scene" else (w <= 48 and h <= 27 and b <= 4 and (spp <= 3 or (spp == 64 and w * h <= 35))), op


def test_the_committed_sequences_cover_every_transition():
    """Every transition the module claims holds at least once in the committed seeds, as a predicate over the model's records; what
    runs of deliberately broken builds need holds in a seed of one sphere count and one cubemap dimension."""
    seen = {}
    for seed in SEEDS:
        records = run_model(seed).records
        for name in sorted(transitions_of(records)):
            seen.setdefault(name, []).append(seed)
        if seed % 4 == 0:
            assert len({r["n"] for r in records}) == 1 and len({r["frame"]["sky"].shape[1] for r in records if "frame" in r}) == 1, seed
        assert sum(r["kind"] == "count" and r["op"][1] == BIG for r in records) <= 1, f"seed {seed}: the scene beyond LDS more than once"
    print("transitions and the seeds that cover them:")
    for name in TRANSITIONS:
        print(f"  {name}: {seen.get(name, [])}")
    missing = sorted(set(TRANSITIONS) - set(seen))
    assert not missing, f"no committed seed contains: {missing}"
    for name in UNIFORM_TRANSITIONS:
        assert any(s % 4 == 0 for s in seen[name]), name


def moving_from_history(records, k):
    """trt_scene_is_moving() after record k, from the history alone: the latest of the events that set or clear the flag"""
    start = max([i for i in range(k + 1) if records[i]["kind"] == "shutdown"], default=-1)
    if records[k]["kind"] == "shutdown":
        return False
    for i in range(k, start, -1):
        r = records[i]
        if r["kind"] == "policy" and r["code"] == 0 and r["op"][1] == 0:
            return False
        if not _called(r):
            continue
        run = 0
        for p in reversed(records[start + 1:i + 1]):  # the run of equal outcomes that ends with call i
            if _called(p):
                if p["changed"] != r["changed"]:
                    break
                run += 1
        if r["changed"] and 0 < r["policy"][0] <= run:
            return True
        if not r["changed"] and run >= r["policy"][1]:
            return False
    return False


def test_the_model_agrees_with_a_stand_in_of_the_policy():
    """The model keeps the two run counters as the library does.  Here the flag and the builds are recomputed from the records'
    history alone -- which calls changed, which policy was in force -- and must agree with what the model recorded."""
    for seed in SEEDS:
        records = run_model(seed).records
        cheap = None  # were the tables in place built for a moving scene
        for k, r in enumerate(records):
            assert r["moving"] == moving_from_history(records, k), (seed, k, r["op"])
            if r["kind"] == "shutdown":
                cheap = None
            if _called(r):
                build = cheap is None or r["changed"] or cheap != r["moving"]
                assert r["builds"] == int(build), (seed, k, r["op"])
                cheap = r["moving"] if build else cheap
            else:
                assert r["builds"] == 0
            assert r["total"] == (0, 0) or r["ctx_after"]


def _scene_data(snap, camera):
    return S.SceneData(snap["spheres"], snap["ground"], snap["dir"], snap["point"], camera, snap["sky"])


def camera_of(cam, w, h):
    """the stored camera of the animation at index cam[1]; cam[2]: turned about its own y axis with the eye where it was"""
    from test_ansi_text import anim_cameras
    c = anim_cameras([cam[1]], w, h)[0]
    c[12] = 3.0  # the screen three times as far from the eye: at 48 x 27 a sphere of the stage is several pixels across
    if cam[2]:
        x, z, a = c[0:3].copy(), c[6:9].copy(), 0.3
        c[0:3], c[6:9] = np.cos(a) * x + np.sin(a) * z, np.cos(a) * z - np.sin(a) * x
    return c


def test_every_edit_is_visible_in_the_oracles_frames():
    """The guard against testing nothing: for every edit of every committed seed, the oracle's frame of the scene after the edit
    differs from its frame of the scene before it, at the camera and shape of the call that follows the edit.  (Edits that are
    NOT to be seen by the policy -- the same texels behind new pointers -- are the exception and are named here.)"""
    import support as T
    edits = 0
    for seed in SEEDS:
        records = run_model(seed).records
        for k, r in enumerate(records):
            if "before" not in r or r["op"][:2] == ("sky_new", "same"):
                continue
            call = next((p for p in records[k + 1:] if _good(p)), None)
            if call is None:
                continue
            w, h, b, spp = call["shot"]
            cam = camera_of(call["cam"], w, h)
            before, _ = T.oracle_render(_scene_data(r["before"], cam), w, h, b, spp)
            after, _ = T.oracle_render(_scene_data(r["after"], cam), w, h, b, spp)
            assert not np.array_equal(before.view(np.uint64), after.view(np.uint64)), f"seed {seed}, step {k}: {r['op']} does not show in the frame of {call['op']}"
            edits += 1
    print(f"{edits} edits, every one visible")
    assert edits >= 10 * len(SEEDS)


# ---- on the GPU ----

def describe(seed, step, ops):
    return (f"seed {seed}, step {step}: {ops[step]}\nreproduce: python -m pytest tests/test_dropin_sequences.py -m gpu -k 'replayed and seed{seed}'\n"
            "operations so far:\n" + "\n".join(f"  {k:3d} {op}" for k, op in enumerate(ops[:step + 1])))


class Replay:
    """drives the drop-in entries through a sequence beside the model; the model's own arrays are the caller's scene, so an edit in
    place reaches the library through the pointers it has seen before, and every cubemap a caller ever held stays allocated"""

    def __init__(self, seed):
        import support as T
        from terminalraytracer_amd import hip
        from terminalraytracer_amd import layout as L
        from test_ansi_text import emitter_text
        self.T, self.hip, self.L, self.emitter_text = T, hip, L, emitter_text
        self.lib = hip.lib()
        self.seed = seed
        self.model = Model(make_pool(seed))
        self.oracle = {}

    def want(self, rec):
        snap, (w, h, b, spp) = rec["frame"], rec["shot"]
        key = (tuple(zlib.crc32(snap[k].tobytes()) for k in ("spheres", "ground", "dir", "point", "sky")), snap["sky"].shape[1], rec["cam"], rec["shot"])
        if key not in self.oracle:
            px, _ = self.T.oracle_render(_scene_data(snap, camera_of(rec["cam"], w, h)), w, h, b, spp)
            assert np.isfinite(px).all(), "the oracle's frame is not finite"
            self.oracle[key] = px
        return self.oracle[key]

    def scene_struct(self, rec):
        m, (w, h) = self.model, rec["shot"][:2]
        data = self.S_data = S.SceneData(m.spheres, m.ground, m.dir, m.point, camera_of(rec["cam"], w, h), m.skies[m.sky])
        assert data.sky.ctypes.data == m.skies[m.sky].ctypes.data and (not len(m.spheres) or data.spheres.ctypes.data == m.spheres.ctypes.data)
        scene, L = data.as_scene(), self.L
        bad = rec.get("bad")
        if bad == "null_array":
            scene.spheres = C.POINTER(L.Sphere)()
        elif bad == "negative_count":
            scene.num_directional_lights = -1
        elif bad == "dim0":
            scene.skybox.dim = 0
        elif bad == "null_face":
            scene.skybox.colors[3] = C.POINTER(L.Color)()
        return scene

    def call(self, rec):
        """(return code, what the entry wrote)"""
        lib, entry, (w, h, b, spp) = self.lib, rec["entry"], rec["shot"]
        scene = self.scene_struct(rec)
        if entry in ("project_scene", "trt_render_frame", "render_frame"):
            screen, out = S.new_screen(w, h)
            if entry == "project_scene":
                lib.project_scene(C.byref(scene), C.byref(screen))
                return 0, out
            return getattr(lib, entry)(C.byref(scene), C.byref(screen), b, spp), out
        if entry == "trt_render_frame_rgb8":
            out = np.zeros((h, w, 3), dtype=np.uint8)
            return lib.trt_render_frame_rgb8(C.byref(scene), w, h, b, spp, out.ctypes.data), out
        out = np.zeros(self.hip.ansi_bytes(w, h), dtype=np.uint8)
        return lib.trt_render_frame_ansi(C.byref(scene), w, h, b, spp, out.ctypes.data), out

    def step(self, i, ops):
        lib, op = self.lib, ops[i]
        rec = self.model.apply(op)
        where = describe(self.seed, i, ops)
        kind, code = op[0], 0
        if kind in ("render", "bad"):
            if rec["code"] == 0:
                want = self.want(rec)  # before anything is launched
            code, got = self.call(rec)
            if code == HIP:
                pytest.fail(f"HIP error, the sequence stops here: {lib.trt_last_error().decode()}\n{where}", pytrace=False)
            assert code == rec["code"], f"code {code} ({lib.trt_last_error().decode()}) where the model expects {rec['code']}\n{where}"
            if code == 0:
                if rec["entry"] == "trt_render_frame_rgb8":
                    want = self.T.oracle_rgb8(want)
                elif rec["entry"] == "trt_render_frame_ansi":
                    want = self.emitter_text(self.T.oracle_rgb8(want))
                else:
                    got, want = got.view(np.uint64), want.view(np.uint64)
                assert got.shape == want.shape, where
                wrong = int((got != want).sum())
                assert not wrong, f"{rec['entry']}: {wrong} of {want.size} values differ from the oracle's\n{where}"
        elif kind == "policy":
            code = lib.trt_set_scene_policy(op[1], op[2])
        elif kind == "shutdown":
            code = lib.trt_shutdown()
        elif kind == "init":
            code = lib.trt_init(0)
        elif kind == "invalidate":
            code = lib.trt_invalidate_skybox()
        elif kind == "upload_skybox":
            if op[1] == "null":
                code = lib.trt_upload_skybox(None)
            else:
                m = self.model
                scene = S.SceneData(m.spheres, m.ground, m.dir, m.point, np.zeros(15), m.skies[m.sky]).as_scene()
                code = lib.trt_upload_skybox(C.byref(scene.skybox))
        if code == HIP:
            pytest.fail(f"HIP error, the sequence stops here: {lib.trt_last_error().decode()}\n{where}", pytrace=False)
        assert code == rec["code"], f"code {code} where the model expects {rec['code']}\n{where}"
        assert lib.trt_scene_is_moving() == int(rec["moving"]), f"trt_scene_is_moving() is {lib.trt_scene_is_moving()}, the model expects {int(rec['moving'])}\n{where}"
        ctx = self.hip.default_context()
        assert (ctx is not None) == rec["ctx_after"], f"trt_default_context() is {'not ' if ctx else ''}NULL\n{where}"
        if ctx is not None:
            counts = ctx.build_counts()
            assert counts == rec["total"], (f"(table builds, skybox uploads) so far {counts}, the model expects {rec['total']}: this call performs "
                                            f"{rec['builds']} and {rec['uploads']}\n{where}")
            if rec["patches"] is not None and rec["code"] == 0:
                assert ctx.path_patches() == rec["patches"], f"path_patches() {ctx.path_patches()}, the model expects {rec['patches']}\n{where}"


@gpu
@pytest.mark.parametrize("seed", SEEDS, ids=[f"seed{s}" for s in SEEDS])
def test_a_sequence_replayed_on_the_drop_in_entries(seed):
    from terminalraytracer_amd import hip
    lib = hip.lib()
    ops = make_sequence(seed)
    replay = Replay(seed)
    t0 = time.perf_counter()
    hip._check(lib.trt_shutdown())  # a fresh default context: earlier tests have handed the drop-in entries other scenes
    hip._check(lib.trt_set_scene_policy(*DEFAULT_POLICY))
    try:
        for i in range(len(ops)):
            replay.step(i, ops)
    finally:
        lib.trt_set_scene_policy(*DEFAULT_POLICY)
        lib.trt_shutdown()
    print(f"seed {seed}: {len(ops)} operations, {len(replay.oracle)} oracle frames, {time.perf_counter() - t0:.2f} s")
