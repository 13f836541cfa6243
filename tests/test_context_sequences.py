"""A seeded model test of the context API: what a trt_context keeps between calls -- jitter table and screen axes, the eye tables of
the single frames and of a batch's slots, the queue a frame leaves ready, occupancy figures, grow-only buffers, the variant it
reports from -- is exercised AGAINST ONE ANOTHER by generated sequences of calls, and every frame any of them produces must be, bit
for bit, the CPU oracle's for the scene, camera, refraction and rows the MODEL says are current.

make_sequence(seed, steps) is pure (numpy only): plain-data operations, made of scripted motifs (the transitions the module claims
to cover, TRANSITIONS) woven into random calls, drawn from a small per-seed set of scenes, cameras and frame shapes so that the same
eye recurs in the same slot and the same launch shape recurs across scene and table changes.  Model follows a sequence without a
GPU: what every operation must return or render, and one record per operation; the transitions are predicates over those records.
  * test_the_committed_sequences_cover_every_transition   (no GPU) every name in TRANSITIONS holds somewhere in the committed seeds
  * test_a_sequence_replayed_on_real_contexts             (gpu)    the replay; reproduce one seed with  -k "replayed and seed7"
Counters are compared after every synchronous render, and for an asynchronous one at the synchronize that follows it when no other
render came between (a later render clears them); a shard rendered with the refraction extension has no oracle count.
Seeds with seed % 4 == 0 draw their scenes from one sphere count (no demo scene, no scene beyond LDS): a stale candidate list can
then never name a sphere the current scene lacks, which is what runs of deliberately broken builds need."""
import numpy as np
import pytest

gpu = pytest.mark.gpu
HIP, ARGUMENT, NO_SCENE, CAPACITY = -1, -2, -3, -4
SEEDS = tuple(range(16))
STEPS = 44
SPLIT_SPHERES = 278  # a batch of 8 is split for LDS at 276 / 278 / 280 spheres without patches (profiles/r07/a_batch.md)
DEFAULT_TABLES = {"path_grids": (64, 32), "path_patches": (-1,), "path_grids_min_spheres": (12,), "light_grids": (128, 64), "light_slabs": (16, 16)}
SETTER_VALUES = {"path_grids": ((64, 32), (16, 8), (40, 32), (0, 0)), "path_patches": ((-1,), (0,), (1,), (2,)),
                 "path_grids_min_spheres": ((12,), (0,), (100,)), "light_grids": ((128, 64), (0, 0), (33, 7)), "light_slabs": ((16, 16), (1, 1), (5, 3))}
SETTERS = tuple(SETTER_VALUES)
SINGLES = ("render_host", "render_host_rgb8", "render_device")
BATCHES = ("render_host_batch", "render_device_batch", "batch_on_former_sharer")


# ---- the pool of a seed: scenes, cameras, frame shapes (plain data) ----

def make_pool(seed):
    rng = np.random.default_rng(7000 + seed)
    if seed % 4 == 0:  # one sphere count throughout
        n = int(rng.choice([24, 64, 150]))
        scenes = [("synth", n, 11 + seed), ("synth", n, 12 + seed), ("lights", n, int(rng.integers(3, 7)), 13 + seed)]
    else:
        dense = {1: SPLIT_SPHERES, 2: int(rng.choice([256, 257])), 3: int(rng.integers(129, 301))}[seed % 4]
        scenes = [("demo",), ("synth", int(rng.integers(12, 128)), 21 + seed), ("synth", dense, 17),
                  ("lights", int(rng.integers(24, 65)), int(rng.integers(3, 7)), 23 + seed), ("big", 1500, 5)]
    anim = [int(i) for i in rng.choice(60, size=3, replace=False)]
    cams = [("anim", anim[0]), ("anim", anim[1]), ("anim", anim[2]), ("bench", float(rng.choice([0.5, 2.5, 10.0])))]

    def rows_of(h):
        if h < 9 or rng.random() < 0.5:
            return ("whole",)
        world = int(rng.integers(2, 4))
        return ("shard", int(rng.integers(0, world)), world, int(rng.choice([1, 4])))

    def shot(size, spps):
        w, h = size
        return (w, h, rows_of(h), int(rng.integers(1, 9)), int(rng.choice(spps)))

    pick = lambda sizes: tuple(int(v) for v in sizes[int(rng.integers(len(sizes)))])
    shots = [shot((1, 1), [1, 2, 3, 10]),                       # one pixel: width 1, a single row, fewer samples than a wave
             shot(pick([(7, 1), (1, 9)]), [1, 2, 3]),
             (5, 3, ("whole",), int(rng.integers(1, 9)), 2),    # 30 samples a frame: eight frames of it in four waves
             shot(pick([(20, 11), (32, 18)]), [10, 64]),
             shot(pick([(67, 13), (32, 18), (33, 17)]), [3, 10]),
             shot((96, 54), [1, 2, 3]),
             (96, 54, ("whole",), 2, 64)]                       # 331 776 samples a frame: a batch outruns the chunks its waves own
    return {"seed": seed, "scenes": scenes, "cams": cams, "shots": shots, "small_shots": 4}  # the first four are at most 32 x 18


def spheres_of(spec):
    return 6 if spec[0] == "demo" else spec[1]


def owned_rows(h, rows):
    if rows[0] == "whole":
        return list(range(h))
    _, rank, world, tile = rows
    tiles = (h + tile - 1) // tile
    return [t * tile + r for t in range(rank, tiles, world) for r in range(min(tile, h - t * tile))]


# ---- the model ----

class ModelContext:
    def __init__(self, group):
        self.group, self.slot, self.scene = group, 0, None
        self.tables = dict(DEFAULT_TABLES)
        self.kernel, self.counters, self.compaction, self.scene_image, self.ior = 0, False, -1, -1, False
        self.stream, self.reserve, self.scratch = "own", 0, 0


class Model:
    """What the library must do with a sequence, and a record per operation for the transition predicates."""

    def __init__(self, pool):
        self.pool = pool
        self.groups = 1
        self.ctx = {0: ModelContext(0)}
        self.main = 0
        self.outstanding = 0
        self.records = []

    # -- what the model knows --
    def shared(self, j):
        return sum(1 for c in self.ctx.values() if c.group == self.ctx[j].group) > 1

    def sharers(self):
        return sorted(j for j in self.ctx if j != self.main)

    def free_ids(self):
        return [j for j in range(3) if j not in self.ctx]

    def spec(self, j):
        return self.pool["scenes"][self.ctx[j].scene]

    def path_tables(self, j):
        c, n = self.ctx[j], spheres_of(self.spec(j))
        return min(c.tables["path_grids"]) >= 2 and c.tables["path_grids_min_spheres"][0] <= n <= 1024  # TRT_PATH_MAX_SPHERES

    def per_camera(self, j):
        """the model KNOWS the batch has no BATCH form: one launch per camera"""
        c = self.ctx[j]
        return c.counters or c.ior or c.kernel == 1 or self.device_image(j) is True or self.shared(j)

    def device_image(self, j):
        """True / False where the model can know where the kernel reads the scene from, else None"""
        c, spec = self.ctx[j], self.spec(j)
        if c.ior:
            return False  # the refraction extension stages the scene in LDS only
        if c.scene_image == 1 or (spec[0] == "big" and c.scene_image == -1):
            return True
        if c.scene_image == -1 and c.kernel == 0 and spheres_of(spec) <= 128:
            return False
        return None

    # -- one operation --
    def apply(self, op):
        kind = op[0]
        j = self.main
        rec = {"op": op, "kind": kind, "code": 0, "ctx": j, "frames": [], "changed": False}
        if kind == "set_scene":
            c = self.ctx[j]
            assert not c.ior, "the generator turns the refraction off before it changes the scene"
            if self.shared(j):  # tables of its own again
                c.group, c.slot = self.groups, 0
                self.groups += 1
            rec["changed"] = c.scene != op[1]
            c.scene = op[1]
        elif kind in SETTERS or kind == "setter_on_sharer":
            who, which, value = (op[1], op[2], op[3]) if kind == "setter_on_sharer" else (j, kind, op[1])
            rec["ctx"], rec["setter"] = who, which
            if self.shared(who):
                rec["code"] = ARGUMENT
            else:
                rec["changed"] = self.ctx[who].tables[which] != value
                self.ctx[who].tables[which] = value
        elif kind in ("set_compaction", "set_scene_image", "set_kernel", "enable_counters", "set_refraction", "set_stream", "reserve_cus"):
            attr = {"set_compaction": "compaction", "set_scene_image": "scene_image", "set_kernel": "kernel", "enable_counters": "counters",
                    "set_refraction": "ior", "set_stream": "stream", "reserve_cus": "reserve"}[kind]
            assert not (kind == "set_kernel" and op[1] == 1 and self.ctx[j].ior) and not (kind == "set_refraction" and op[1] and self.ctx[j].kernel == 1), \
                "the reference-order kernel and the refraction extension are not combined"
            setattr(self.ctx[j], attr, op[1])
        elif kind == "synchronize":
            self.outstanding = 0
        elif kind == "close":
            rec["ctx"] = op[1]
            del self.ctx[op[1]]
        elif kind == "share":
            who, cam, shot = op[1], op[2], op[3]
            if who not in self.ctx:
                self.ctx[who] = ModelContext(-1)
            d, s = self.ctx[who], self.ctx[j]
            if d.group != s.group:
                d.group = s.group
                d.slot = min(k for k in range(8) if k not in {c.slot for i, c in self.ctx.items() if c.group == s.group and i != who})
                d.scene, d.tables, d.ior = s.scene, dict(s.tables), False
            rec["ctx"] = who
            self._render(rec, who, [cam], shot, batch=False)
        elif kind == "adopt":  # the main context gives up its tables and shares those a former sharer was left with
            d, s = self.ctx[j], self.ctx[op[1]]
            assert d.group != s.group and not d.ior
            d.group = s.group
            d.slot = min(k for k in range(8) if k not in {c.slot for i, c in self.ctx.items() if c.group == s.group and i != j})
            d.scene, d.tables = s.scene, dict(s.tables)
        elif kind in SINGLES:
            self._render(rec, j, [op[1]], op[2], batch=False)
        elif kind in ("render_host_batch", "render_device_batch"):
            self._render(rec, j, list(op[1]), op[2], batch=True)
        elif kind == "batch_on_former_sharer":
            self.outstanding = 0  # the replay collects what is outstanding before it closes the source
            for other in [i for i in self.ctx if i != op[1]]:
                del self.ctx[other]
            self.main = rec["ctx"] = op[1]
            self._render(rec, op[1], list(op[2]), op[3], batch=True)
        else:
            raise AssertionError(kind)
        if kind in ("render_device", "render_device_batch") and rec["code"] == 0:
            self.outstanding += 1
        self.records.append(rec)
        return rec

    def _render(self, rec, j, cams, shot, batch):
        c, spec = self.ctx[j], self.spec(j)
        w, h, rows, b, spp = shot
        n = len(cams)
        pixels = len(owned_rows(h, rows)) * w
        rec.update(scene=c.scene, spec=spec, cams=cams, shot=shot, n=n, pixels=pixels, units=pixels * spp, slot=c.slot, stream=c.stream, reserve=c.reserve,
                   counters=c.counters, ior=c.ior, kernel=c.kernel, scene_image=c.scene_image, compaction=c.compaction, shared=self.shared(j),
                   path_tables=self.path_tables(j), tables=dict(c.tables), device_image=self.device_image(j), batch=batch, grows_scratch=False)
        if batch and n > 1 and self.shared(j):
            rec["code"] = CAPACITY
        elif c.ior and spec[0] == "big":
            rec["code"] = CAPACITY  # no device-image form of the refraction extension
        if rec["code"]:
            rec["fused"] = False
            return
        rec["frames"] = [(c.scene, cam, c.ior) for cam in cams]
        rec["fused"] = batch and not self.per_camera(j)
        rec["launches"] = ("equal", n) if batch and self.per_camera(j) else ("between", 1, n)
        if c.kernel == 0:
            need = pixels * spp * (n if rec["fused"] else 1)
            rec["grows_scratch"], c.scratch = need > c.scratch, max(c.scratch, need)


# ---- the transitions: predicates over (records before, this record) ----

def _fused(r):
    return r["kind"] in BATCHES and r["code"] == 0 and r["fused"]


def _previous_fused(hist, rec):
    """(index, record) of the BATCH launch before this one on the same context"""
    for i in range(len(hist) - 1, -1, -1):
        if _fused(hist[i]) and hist[i]["ctx"] == rec["ctx"]:
            return i, hist[i]
    return None, None


def _same_eye_slots(p, rec, tables=True):
    """slots other than the single frames' whose eye both batches have in common (with the path tables on in both)"""
    if tables and not (p["path_tables"] and rec["path_tables"]):
        return []
    return [b for b in range(min(p["n"], rec["n"])) if p["cams"][b] == rec["cams"][b] and b != rec["slot"]]


def _between(hist, rec, test, same_context=True):
    i, p = _previous_fused(hist, rec)
    return _fused(rec) and p is not None and any(test(r) for r in hist[i + 1:] if not same_context or r["ctx"] == rec["ctx"])


def t_scene_change_same_eyes(hist, rec):
    """1: a batch after trt_set_scene to ANOTHER scene, at least one slot's eye as in the batch before"""
    _, p = _previous_fused(hist, rec)
    return _fused(rec) and p is not None and p["scene"] != rec["scene"] and bool(_same_eye_slots(p, rec))


def _t_setter(which):
    def t(hist, rec):
        i, p = _previous_fused(hist, rec)
        return (_fused(rec) and p is not None and p["scene"] == rec["scene"] and bool(_same_eye_slots(p, rec, tables=which.startswith("light")))
                and any(r.get("setter") == which and r["code"] == 0 and r["changed"] and r["ctx"] == rec["ctx"] for r in hist[i + 1:]))
    t.__doc__ = f"2: trt_set_{which} (accepted, another value) between two batches of one scene with an eye in common in a slot"
    return t


def t_batch_on_nonzero_eye_slot(hist, rec):
    """3: a batch on a former sharer: the context's own eye slot is not 0 and is one of the batch's"""
    return _fused(rec) and rec["path_tables"] and 0 < rec["slot"] < rec["n"]


def t_sharer_used_a_slot_between(hist, rec):
    """4: source batch; a sharer takes one of its slots, renders ANOTHER eye there and closes; the same batch again"""
    i, p = _previous_fused(hist, rec)
    if not _fused(rec) or p is None or p["scene"] != rec["scene"]:
        return False
    for k in range(i + 1, len(hist)):
        s = hist[k]
        if s["kind"] == "share" and s["code"] == 0 and s["slot"] in _same_eye_slots(p, rec) and s["cams"][0] != rec["cams"][s["slot"]] \
                and any(r["kind"] == "close" and r["ctx"] == s["ctx"] for r in hist[k + 1:]):
            return True
    return False


def _t_back_to_back(what):
    def t(hist, rec):
        if not hist or rec["kind"] != "render_device_batch" or hist[-1]["kind"] != "render_device_batch" or not (_fused(rec) and _fused(hist[-1])):
            return False
        p = hist[-1]
        return {"cameras": p["cams"] != rec["cams"], "n": p["n"] != rec["n"], "spp": p["shot"][4] != rec["shot"][4],
                "scratch": rec["grows_scratch"] and p["shot"][:3] != rec["shot"][:3]}[what]
    t.__doc__ = f"5: trt_render_device_batch straight after another with nothing between them, differing in: {what}"
    return t


def t_batch_on_user_stream(hist, rec):
    """6: a batch on the caller's stream"""
    return _fused(rec) and rec["stream"] == "user"


def t_batch_after_stream_returned(hist, rec):
    """6: ... and the next batch on the context's own stream again"""
    _, p = _previous_fused(hist, rec)
    return _fused(rec) and rec["stream"] == "own" and p is not None and p["stream"] == "user"


def t_batch_with_reserved_cus(hist, rec):
    """6: a batch with trt_reserve_cus in force"""
    return _fused(rec) and rec["stream"] == "own" and rec["reserve"] > 0


def _t_detour(name, test):
    def t(hist, rec):
        return _between(hist, rec, lambda r: r["kind"] in BATCHES and r["code"] == 0 and test(r))
    t.__doc__ = f"7: BATCH launch, then a batch served per camera because of {name}, then a BATCH launch again"
    return t


def _plain_rounds(r):
    """a frame or batch of the plain 256-thread rounds on tables without patches, on the context's own stream"""
    return (not (r["counters"] or r["ior"] or r["kernel"] or r["device_image"]) and r["compaction"] != 1 and r["path_tables"]
            and r["tables"]["path_patches"] == (0,) and r["stream"] == "own")


def splits_for_lds(r):
    """a batch of 8 the model expects LDS to split: no patches and a sphere count of the split band (profiles/r07/a_batch.md); the
    replay asserts that it was split, so that a moved threshold cannot quietly drop the transition below"""
    return (_fused(r) and r["n"] == 8 and r["spec"][0] == "synth" and 276 <= r["spec"][1] <= 280 and r["shot"][4] <= 3 and _plain_rounds(r))


def t_split_batch_then_single_of_its_shape(hist, rec):
    """7: a batch of 8 that LDS splits (no patches, a sphere count of the split band), every launch one workgroup, then a single
    frame of the same shape: its queue shape equals the split's last launch"""
    if not hist or rec["kind"] not in SINGLES or rec["code"] or rec["ctx"] != hist[-1]["ctx"]:
        return False
    p = hist[-1]
    return splits_for_lds(p) and p["units"] * 8 <= 256 and _plain_rounds(rec) and rec["shot"] == p["shot"] and rec["scene"] == p["scene"]


def t_batch_after_adopting_other_tables(hist, rec):
    """1, 3, 4 together: a context that has batched on tables of its own adopts the tables a former sharer was left with (another
    scene, whose slots hold other eyes), the sharer closes, and the batch has the eyes of the context's batch before in its slots"""
    i, p = _previous_fused(hist, rec)
    return (_fused(rec) and p is not None and bool(_same_eye_slots(p, rec)) and p["scene"] != rec["scene"]
            and any(r["kind"] == "adopt" for r in hist[i + 1:]) and not any(r["kind"] == "set_scene" for r in hist[i + 1:]))


def effective_patches(r):
    m = r["tables"]["path_patches"][0]
    return (2 if spheres_of(r["spec"]) >= 128 else 0) if m < 0 else m


def t_queue_words_change_between_batches_of_one_shape(hist, rec):
    """7: two BATCH launches of one shape (frames, size, rays per pixel) and OTHER cameras, so large that their waves ask the queue
    for work (more than 600 000 samples: the workgroups that fit the device own fewer chunks than that), and between them nothing
    but a trt_set_path_patches that takes the spheres' patches away: the queue's one word becomes a word per XCD"""
    if len(hist) < 2 or not _fused(rec) or not _fused(hist[-2]) or hist[-1].get("setter") != "path_patches" or hist[-1]["code"]:
        return False
    p = hist[-2]
    return (p["ctx"] == rec["ctx"] and p["shot"] == rec["shot"] and p["n"] == rec["n"] and p["cams"] != rec["cams"] and p["scene"] == rec["scene"]
            and rec["units"] * rec["n"] >= 600000 and rec["path_tables"] and p["path_tables"]
            and effective_patches(p) > 0 and effective_patches(rec) == 0 and rec["compaction"] != 1 and p["compaction"] != 1
            and rec["stream"] == p["stream"] and rec["reserve"] == p["reserve"])


def t_wave_holds_several_frames(hist, rec):
    """8: a BATCH launch of frames of fewer than 64 samples each"""
    return _fused(rec) and rec["n"] >= 2 and rec["units"] < 64


def t_batch_of_width_one(hist, rec):
    """8: ... of frames one pixel wide"""
    return _fused(rec) and rec["n"] >= 2 and rec["shot"][0] == 1


def t_batch_of_a_single_row(hist, rec):
    """8: ... of frames of a single row"""
    return _fused(rec) and rec["n"] >= 2 and rec["shot"][1] == 1


TRANSITIONS = {"scene_change_same_eyes": t_scene_change_same_eyes}
TRANSITIONS.update({f"{which}_between_same_batches": _t_setter(which) for which in SETTERS})
TRANSITIONS.update({"batch_on_nonzero_eye_slot": t_batch_on_nonzero_eye_slot, "sharer_used_a_slot_between": t_sharer_used_a_slot_between})
TRANSITIONS.update({f"device_batches_back_to_back_other_{what}": _t_back_to_back(what) for what in ("cameras", "n", "spp", "scratch")})
TRANSITIONS.update({"batch_on_user_stream": t_batch_on_user_stream, "batch_after_stream_returned": t_batch_after_stream_returned,
                    "batch_with_reserved_cus": t_batch_with_reserved_cus,
                    "batch_device_image_scene_batch": _t_detour("a scene beyond LDS", lambda r: r["spec"][0] == "big" and r["device_image"] is True),
                    "batch_refraction_batch": _t_detour("the refraction extension", lambda r: r["ior"]),
                    "batch_counters_batch": _t_detour("the counters", lambda r: r["counters"]),
                    "batch_scene_image_1_batch": _t_detour("trt_set_scene_image(1)", lambda r: r["scene_image"] == 1 and r["device_image"] is True),
                    "batch_reference_kernel_batch": _t_detour("the reference-order kernel", lambda r: r["kernel"] == 1),
                    "split_batch_then_single_of_its_shape": t_split_batch_then_single_of_its_shape,
                    "batch_after_adopting_other_tables": t_batch_after_adopting_other_tables,
                    "queue_words_change_between_batches_of_one_shape": t_queue_words_change_between_batches_of_one_shape,
                    "wave_holds_several_frames": t_wave_holds_several_frames, "batch_of_width_one": t_batch_of_width_one,
                    "batch_of_a_single_row": t_batch_of_a_single_row})


def transitions_of(records):
    return {name for k, rec in enumerate(records) for name, test in TRANSITIONS.items() if test(records[:k], rec)}


# ---- the generator ----

def make_sequence(seed, steps=STEPS):
    """At least `steps` plain-data operations for the pool of `seed`; deterministic; no GPU."""
    pool = make_pool(seed)
    rng = np.random.default_rng(9000 + seed)
    model = Model(pool)
    ops = []
    scenes, cams, shots = pool["scenes"], pool["cams"], pool["shots"]
    small = [k for k, s in enumerate(scenes) if s[0] != "big"]
    big = [k for k, s in enumerate(scenes) if s[0] == "big"]

    def emit(*op):
        ops.append(op)
        return model.apply(op)

    me = lambda: model.ctx[model.main]
    pick = lambda seq: seq[int(rng.integers(len(seq)))]

    def shot(tiny=False):
        if tiny:
            return shots[int(rng.integers(0, 3))]
        few = model.spec(model.main)[0] == "big"  # frames of the scene beyond LDS stay at or below 32 x 18; the last shot is m_queue_words' own
        return shots[int(rng.integers(0, pool["small_shots"] if few else len(shots) - 1))]

    def lineup(n=None, start=None):
        """the cameras of a batch: a run of the seed's few cameras, so that an eye keeps its slot from batch to batch"""
        n = int(rng.integers(2, 9)) if n is None else n
        start = int(rng.random() < 0.25) if start is None else start
        return tuple(cams[(start + i) % len(cams)] for i in range(n))

    def drain():
        if model.outstanding:
            emit("synchronize")

    def unshare():
        for j in model.sharers():
            emit("close", j)

    def clean(scene=None):
        """a context whose batches are BATCH launches: nothing shared, no counters, refraction, reference kernel or device image"""
        unshare()
        if me().ior:
            emit("set_refraction", False)
        if me().counters:
            emit("enable_counters", False)
        if me().kernel:
            emit("set_kernel", 0)
        if me().scene_image != -1:
            emit("set_scene_image", -1)
        if scene is not None and me().scene != scene:
            emit("set_scene", scene)
        elif me().scene is None or model.spec(model.main)[0] == "big":
            emit("set_scene", pick(small))
        if not model.path_tables(model.main) and spheres_of(model.spec(model.main)) >= 12:
            emit("path_grids", DEFAULT_TABLES["path_grids"])
            if not model.path_tables(model.main):
                emit("path_grids_min_spheres", (12,))

    def batch(cameras, s, device=None):
        device = rng.random() < 0.3 if device is None else device
        if device and model.outstanding >= 3:
            drain()
        emit("render_device_batch" if device else "render_host_batch", cameras, s)

    def tabled_scene():
        return pick([k for k in small if spheres_of(scenes[k]) >= 12])

    # -- the motifs: each is one of the transitions the module claims --
    def m_scene_swap():
        clean(tabled_scene())
        c, s = lineup(start=0), shot()
        batch(c, s)
        emit("set_scene", pick([k for k in small if k != me().scene and spheres_of(scenes[k]) >= 12]))
        batch(c, s)

    def m_setter():
        which = pick(SETTERS)
        clean(tabled_scene())
        if which.startswith("path") and me().tables[which] != DEFAULT_TABLES[which]:
            emit(which, DEFAULT_TABLES[which])
        c, s = lineup(start=0), shot()
        batch(c, s)
        values = [v for v in SETTER_VALUES[which] if v != me().tables[which]]
        if which == "path_grids":
            values = [v for v in values if min(v) >= 2]  # the eye slots move with g_eye; (0, 0) turns the tables off altogether
        if which == "path_grids_min_spheres":
            values = [v for v in values if v[0] <= spheres_of(model.spec(model.main))]
        emit(which, pick(values))
        batch(c, s)

    def m_former_sharer():
        clean(tabled_scene())
        drain()
        j = pick(model.free_ids())
        emit("share", j, pick(cams), shot())
        emit("batch_on_former_sharer", j, lineup(n=int(rng.integers(3, 9))), shot())

    def m_sharer_between():
        clean(tabled_scene())
        c, s = lineup(n=int(rng.integers(3, 9)), start=0), shot()
        batch(c, s, device=False)
        j = pick(model.free_ids())
        emit("share", j, c[2], shot())  # slot 1 is the sharer's: the batch's camera there is c[1]
        if rng.random() < 0.5:
            emit("render_host_batch", c, s)  # refused: the tables are shared
        emit("close", j)
        batch(c, s, device=False)

    def m_back_to_back():
        clean()
        drain()
        s = shot()
        n = int(rng.integers(2, 8))
        emit("render_device_batch", lineup(n=n, start=0), s)
        emit("render_device_batch", lineup(n=n, start=1), s)                       # other cameras
        other = pick([x for x in shots[:pool["small_shots"]] if x[4] != s[4]])
        emit("render_device_batch", lineup(n=n + 1, start=0), other)               # another n, other rays per pixel: the jitter table is rewritten
        drain()
        emit("render_device_batch", lineup(n=2, start=0), shots[0])
        emit("render_device_batch", lineup(n=8, start=0), shots[-2])               # the largest frames: the sample scratch grows
        emit("synchronize")

    def m_streams():
        clean()
        c, s = lineup(), shot()
        emit("set_stream", "user")
        batch(c, s)
        if rng.random() < 0.5:
            emit(pick(SINGLES), pick(cams), shot())
        drain()
        emit("set_stream", "own")
        batch(c, s)
        emit("reserve_cus", int(pick([16, 64])))
        batch(lineup(), shot())
        emit(pick(SINGLES), pick(cams), s)
        drain()
        emit("reserve_cus", 0)

    def m_detour():
        what = pick(["counters", "refraction", "kernel", "scene_image"] + (["big"] if big else []))
        clean()
        c, s = lineup(start=0), shot(tiny=what == "big" or rng.random() < 0.3)
        before = me().scene
        batch(c, s)
        on, off = {"counters": (("enable_counters", True), ("enable_counters", False)), "refraction": (("set_refraction", True), ("set_refraction", False)),
                   "kernel": (("set_kernel", 1), ("set_kernel", 0)), "scene_image": (("set_scene_image", 1), ("set_scene_image", -1)),
                   "big": (("set_scene", big[0] if big else 0), ("set_scene", before))}[what]
        emit(*on)
        batch(c, s, device=False if what == "counters" else None)
        if rng.random() < 0.5:
            emit(pick(SINGLES), c[0], s)
        emit(*off)
        batch(c, s)

    def m_split():
        dense = [k for k, sc in enumerate(scenes) if sc[0] == "synth" and 276 <= sc[1] <= 280]
        if not dense:
            return m_tiny()
        clean(dense[0])
        if me().stream != "own":
            emit("set_stream", "own")
        if me().compaction == 1:
            emit("set_compaction", -1)
        if me().tables["path_patches"] != (0,):
            emit("path_patches", (0,))
        batch(lineup(n=8, start=0), shots[2])
        emit(pick(SINGLES), pick(cams), shots[2])
        emit("path_patches", (-1,))

    def m_adopt():
        x = tabled_scene()
        clean(x)
        for which in ("path_grids", "path_grids_min_spheres"):
            if me().tables[which] != DEFAULT_TABLES[which]:
                emit(which, DEFAULT_TABLES[which])
        n, s = int(rng.integers(3, 9)), shot()
        batch(lineup(n=n, start=1), s, device=False)   # the slots of these tables hold the eyes of THIS line-up
        j = pick(model.free_ids())
        emit("share", j, pick(cams), shot())
        drain()
        emit("set_scene", pick([k for k in small if k != x and spheres_of(scenes[k]) >= 12]))  # tables of its own; the sharer keeps the others
        batch(lineup(n=n, start=0), s, device=False)
        drain()
        emit("adopt", j)
        emit("close", j)
        batch(lineup(n=n, start=0), s, device=False)

    def m_queue_words():
        clean(tabled_scene())
        if me().compaction == 1:
            emit("set_compaction", -1)
        s, n = shots[-1], int(rng.integers(2, 4))
        batch(lineup(n=n, start=0), s, device=False)
        emit("path_patches", (0,) if effective_patches(model.records[-1]) > 0 else (2,))
        batch(lineup(n=n, start=1), s, device=False)
        emit("path_patches", (0,) if effective_patches(model.records[-1]) > 0 else (2,))
        batch(lineup(n=n, start=0), s, device=False)  # one of the two changes takes the patches away
        emit("path_patches", (-1,))

    def m_tiny():
        clean()
        for s in (shots[0], shots[1], shots[2]):
            batch(lineup(), s)

    def m_refusals():
        if me().scene is None:
            emit("set_scene", pick(small))
        if not model.sharers():
            emit("share", pick(model.free_ids()), pick(cams), shot())
        j = pick(model.sharers())
        which = pick(SETTERS)
        emit("setter_on_sharer", j, which, pick(SETTER_VALUES[which]))
        emit(which, pick(SETTER_VALUES[which]))                           # ... and on the source: refused on every sharer
        emit("render_host_batch", lineup(), shot())                       # CAPACITY: shared
        emit("render_host_batch", lineup(n=1), shot())                    # one camera always works
        if big and not me().kernel:
            if me().ior:
                emit("set_refraction", False)
            emit("set_scene", big[0])
            emit("set_refraction", True)
            emit(pick(SINGLES), pick(cams), shot())                       # CAPACITY: no device-image form of the extension
            emit("set_refraction", False)
            emit("render_host", pick(cams), shot())

    # -- random calls between the motifs --
    def filler():
        if me().scene is None:
            return emit("set_scene", pick(small))
        kind = pick(["single"] * 6 + ["batch"] * 5 + ["scene"] * 3 + ["setter"] * 3 + ["toggle"] * 4 + ["sync", "share", "close", "stream", "reserve"])
        if kind == "single":
            k = pick(SINGLES)
            if k == "render_device" and model.outstanding >= 3:
                drain()
            emit(k, pick(cams), shot())
        elif kind == "batch":
            c = lineup()
            batch(c if not model.shared(model.main) or rng.random() < 0.2 else c[:1], shot())
        elif kind == "scene":
            if me().ior:
                emit("set_refraction", False)
            emit("set_scene", int(rng.integers(len(scenes))))
        elif kind == "setter":
            which = pick(SETTERS)
            emit(which, pick(SETTER_VALUES[which]))  # refused while the tables are shared
        elif kind == "toggle":
            t = pick(["set_compaction", "set_scene_image", "set_kernel", "enable_counters", "set_refraction"])
            if t == "set_compaction":
                emit(t, int(pick([-1, 0, 1])))
            elif t == "set_scene_image":
                emit(t, int(pick([-1, 1])))
            elif t == "set_kernel":
                emit(t, 0 if me().kernel or me().ior else 1)
            elif t == "enable_counters":
                emit(t, not me().counters)
            elif not me().kernel:
                emit(t, not me().ior)
        elif kind == "sync":
            emit("synchronize")
        elif kind == "share" and model.free_ids():
            emit("share", pick(model.free_ids() + model.sharers()), pick(cams), shot())
        elif kind == "close" and model.sharers():
            emit("close", pick(model.sharers()))
        elif kind == "stream":
            emit("set_stream", "own" if me().stream == "user" else "user")
        elif kind == "reserve":
            emit("reserve_cus", int(pick([0, 16, 64])))

    motifs = [m_scene_swap, m_setter, m_setter, m_former_sharer, m_sharer_between, m_back_to_back, m_streams, m_detour, m_detour, m_split, m_tiny,
              m_refusals, m_adopt, m_queue_words]
    emit("set_scene", pick(small))
    filler()
    motifs[seed % len(motifs)]()  # every motif opens some seed's sequence, whatever the draws below
    if seed % 4 == 1:
        m_split()
    while len(ops) < steps:
        if rng.random() < 0.45:
            motifs[int(rng.integers(len(motifs)))]()
        else:
            filler()
    drain()
    return ops


def run_model(seed):
    model = Model(make_pool(seed))
    for op in make_sequence(seed):
        model.apply(op)
    return model


# ---- without a GPU ----

def test_the_generator_is_deterministic_and_long_enough():
    assert len(SEEDS) >= 12
    for seed in SEEDS:
        first, again = make_sequence(seed), make_sequence(seed)
        assert first == again, seed
        assert len(first) >= 40, (seed, len(first))


def test_the_committed_sequences_cover_every_transition():
    """Every transition the module claims -- points 1 to 8 of what no hand-written scenario exercises -- holds at least once in the
    committed seeds, as a predicate over the model's records; so do the refusals, the pool's scene kinds, the frame sizes and
    rays per pixel."""
    seen, codes, kinds, spps, sizes, scene_kinds = {}, set(), set(), set(), set(), set()
    for seed in SEEDS:
        records = run_model(seed).records
        for name in transitions_of(records):
            seen.setdefault(name, []).append(seed)
        for r in records:
            kinds.add(r["kind"])
            if "shot" in r:
                codes.add((r["kind"] if r["kind"] != "render_host_batch" else "batch", r["code"]))
                if r["code"] == 0:
                    spps.add(r["shot"][4]), sizes.add(r["shot"][:2]), scene_kinds.add(r["spec"][0])
            elif r["code"]:
                codes.add(("setter", r["kind"] == "setter_on_sharer", r["code"]))
        tiny = [r for r in records if r.get("frames") and r["units"] < 64]
        assert tiny, f"seed {seed} renders no frame of fewer than 64 samples"
    print("transitions by seed:", {k: v for k, v in sorted(seen.items())})
    missing = sorted(set(TRANSITIONS) - set(seen))
    assert not missing, f"no committed seed contains: {missing}"
    uniform = [s for s in SEEDS if s % 4 == 0]
    for name in ("scene_change_same_eyes", "sharer_used_a_slot_between", "batch_after_adopting_other_tables"):  # what runs of deliberately broken builds use
        assert set(seen[name]) & set(uniform), name
    assert ("setter", True, ARGUMENT) in codes and ("setter", False, ARGUMENT) in codes and ("batch", CAPACITY) in codes
    assert any(code == CAPACITY and kind in SINGLES for kind, code in (c for c in codes if len(c) == 2)), "refraction on the scene beyond LDS"
    others = {"set_scene", "set_compaction", "set_scene_image", "set_kernel", "enable_counters", "set_refraction", "set_stream", "reserve_cus",
              "synchronize", "share", "close", "setter_on_sharer", "adopt"}
    assert kinds >= set(SINGLES) | set(BATCHES) | set(SETTERS) | others
    assert spps == {1, 2, 3, 10, 64} and (1, 1) in sizes and (96, 54) in sizes and scene_kinds == {"demo", "synth", "lights", "big"}


# ---- on the GPU ----

def describe(seed, step, ops):
    return (f"seed {seed}, step {step}: {ops[step]}\nreproduce: python -m pytest tests/test_context_sequences.py -m gpu -k 'replayed and seed{seed}'\n"
            "operations so far:\n" + "\n".join(f"  {k:3d} {op}" for k, op in enumerate(ops[:step + 1])))


class Replay:
    """drives real contexts through a sequence beside the model and checks everything an operation produces"""

    def __init__(self, seed):
        import support as T
        from terminalraytracer_amd import hip
        from terminalraytracer_amd import scenes as S
        self.T, self.hip, self.S = T, hip, S
        self.seed, self.pool = seed, make_pool(seed)
        self.model = Model(self.pool)
        self.ctx = {}
        self.user_stream = None
        self.pending = []  # (device tensor, record, step)
        self.oracle = {}
        self.anim = np.load(T.GOLDEN + "/cameras_anim.npz")["camera"]
        self.scenes = {}
        self.split_launches = []
        self.last_render = None

    def scene(self, k):
        if k not in self.scenes:
            spec, S, sky, cam = self.pool["scenes"][k], self.S, self.T.sky("synth"), self.camera(self.pool["cams"][0], 16, 9)
            self.scenes[k] = (S.demo_scene(sky, cam) if spec[0] == "demo" else S.synth_scene_lights(spec[1], spec[2], sky, cam, seed=spec[3])
                              if spec[0] == "lights" else S.synth_scene(spec[1], sky, cam, seed=spec[2]))
        return self.scenes[k]

    def ior(self, k):
        n = self.scene(k).num_spheres
        return np.where(np.arange(n) % 3 == 0, 1.5, 0.0)

    def camera(self, cam, w, h):
        if cam[0] == "bench":
            return self.T.bench_camera(w, h, cam[1])
        c = self.anim[cam[1]].copy()
        c[13] = 5 * float(w) / float(h)
        return c

    def rowset(self, shot):
        w, h, rows = shot[:3]
        return self.hip.RowSet.whole(w, h) if rows[0] == "whole" else self.hip.RowSet.shard(w, h, rows[1], rows[2], rows[3])

    def want(self, frame, shot):
        """(owned rows of the oracle's frame, (path rays, shadow rays) of those rows or None), cached by the full key"""
        key = (frame, shot)
        if key not in self.oracle:
            (k, cam, ior), (w, h, rows, b, spp) = frame, shot
            scene = self.scene(k).with_camera(self.camera(cam, w, h))
            owned = owned_rows(h, rows)
            if ior:
                px, st = self.T.oracle_render_refractive(scene, self.ior(k), w, h, b, spp)
                px, stats = px[owned], (st.path_rays, st.shadow_rays) if rows[0] == "whole" else None
            elif rows[0] == "whole":
                px, st = self.T.oracle_render(scene, w, h, b, spp)
                stats = (st.path_rays, st.shadow_rays)
            else:  # the rows of every owned tile, and their rays
                tile = rows[3]
                parts = [self.T.oracle_render(scene, w, h, b, spp, rows=(r0, min(r0 + tile, h))) for r0 in owned if r0 % tile == 0]
                px = np.concatenate([p for p, _ in parts])
                stats = (sum(st.path_rays for _, st in parts), sum(st.shadow_rays for _, st in parts))
            assert np.isfinite(px).all(), "the oracle's frame is not finite"
            self.oracle[key] = (px, stats)
        return self.oracle[key]

    def check_frames(self, got, rec, where):
        bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
        for k, frame in enumerate(rec["frames"]):
            want, _ = self.want(frame, rec["shot"])
            assert got[k].shape == want.shape, f"frame {k}: shape {got[k].shape}, the oracle's {want.shape}\n{where}"
            same = np.array_equal(bits(got[k]), bits(want))
            assert same, f"frame {k} (camera {frame[1]}) differs from the oracle in {int((bits(got[k]) != bits(want)).sum())} of {want.size} values\n{where}"

    def check_counters(self):
        """the counters of the most recent render of all, if it counted: read after a synchronous render, or at the synchronize
        that follows an asynchronous one (a shard of the refraction extension has no oracle count: not compared)"""
        if self.last_render is None:
            return
        c, rec, where = self.last_render
        self.last_render = None
        stats = [self.want(frame, rec["shot"])[1] for frame in rec["frames"]]
        if rec["counters"] and c is self.ctx.get(rec["ctx"]) and all(s is not None for s in stats):
            assert c.read_counters() == tuple(sum(s[k] for s in stats) for k in (0, 1)), "the counters differ from the oracle's\n" + where

    def collect(self, ops):
        for tensor, rec, step in self.pending:
            n, (w, h, rows) = rec["n"], rec["shot"][:3]
            got = tensor.cpu().numpy().reshape(n, len(owned_rows(h, rows)), w, 3)
            self.check_frames(got, rec, "(rendered asynchronously at) " + describe(self.seed, step, ops))
        self.pending = []

    def close_all(self):
        for c in self.ctx.values():
            c.close()
        self.ctx = {}

    def step(self, i, ops):
        import torch
        hip, op = self.hip, ops[i]
        kind = op[0]
        if kind == "batch_on_former_sharer":  # frames in flight on the source are collected before it is closed
            self.ctx[self.model.main].synchronize()
            self.collect(ops)
        rec = self.model.apply(op)
        where = describe(self.seed, i, ops)
        j = rec["ctx"]
        if j not in self.ctx and kind != "close":
            self.ctx[j] = hip.Context(0)
        c = self.ctx.get(j)

        def call(fn):
            """the operation, with the code the model expects"""
            try:
                out = fn()
            except hip.TrtError as e:
                if e.code == HIP:
                    pytest.fail(f"HIP error, the sequence stops here: {e}\n{where}", pytrace=False)
                assert e.code == rec["code"], f"{e} where the model expects code {rec['code']}\n{where}"
                return None
            assert rec["code"] == 0, f"accepted where the model expects code {rec['code']}\n{where}"
            return out

        if kind == "set_scene":
            call(lambda: c.set_scene(self.scene(op[1])))
        elif kind in SETTERS or kind == "setter_on_sharer":
            which, value = rec["setter"], op[3] if kind == "setter_on_sharer" else op[1]
            call(lambda: getattr(c, "set_" + which)(*value))
        elif kind in ("set_compaction", "set_scene_image", "set_kernel", "reserve_cus"):
            call(lambda: getattr(c, kind)(op[1]))
        elif kind == "enable_counters":
            call(lambda: c.enable_counters(op[1]))
        elif kind == "set_refraction":
            call(lambda: c.set_refraction(self.ior(self.model.ctx[j].scene) if op[1] else None))
        elif kind == "set_stream":
            if self.user_stream is None:
                self.user_stream = torch.cuda.Stream(device="cuda:0")
            call(lambda: c.set_stream(self.user_stream.cuda_stream if op[1] == "user" else None))
        elif kind == "synchronize":
            call(c.synchronize)
            self.collect(ops)
            if self.last_render is not None and self.last_render[0] is c:
                self.check_counters()
        elif kind == "close":
            self.ctx.pop(j).close()
        elif kind == "adopt":
            call(lambda: c.share_scene(self.ctx[op[1]]))
        else:
            if kind == "share":
                call(lambda: c.share_scene(self.ctx[self.model.main]))
            if kind == "batch_on_former_sharer":
                for other in [k for k in self.ctx if k != j]:
                    self.ctx.pop(other).close()
            self.render(c, kind, rec, call, where, i)

    def render(self, c, kind, rec, call, where, i):
        import torch
        shot = rec["shot"]
        w, h, rows, b, spp = shot
        rs, n = self.rowset(shot), rec["n"]
        cams = np.stack([self.camera(cam, w, h) for cam in rec["cams"]])
        if rec["code"] == 0:
            for frame in rec["frames"]:
                self.want(frame, shot)  # fails here, before anything is launched, if the oracle's frame is not finite
        got = None
        if kind in ("render_host", "share"):
            got = call(lambda: c.render_host(cams[0], rs, b, spp)[None])
        elif kind == "render_host_rgb8":
            rgb = call(lambda: c.render_host_rgb8(cams[0], rs, b, spp))
            if rgb is not None:
                assert np.array_equal(rgb, self.T.oracle_rgb8(self.want(rec["frames"][0], shot)[0])), "the bytes differ from the oracle's\n" + where
        elif kind in ("render_host_batch", "batch_on_former_sharer"):
            got = call(lambda: c.render_host_batch(cams, rs, b, spp))
        else:
            fb = torch.zeros(max(1, n * rec["pixels"] * 3), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            if kind == "render_device":
                done = call(lambda: c.render_device(cams[0], rs, b, spp, fb.data_ptr(), fb.numel() * 8) or True)
            else:
                done = call(lambda: c.render_device_batch(cams, rs, b, spp, fb.data_ptr(), fb.numel() * 8) or True)
            if done:
                self.pending.append((fb[:n * rec["pixels"] * 3], rec, i))
        if rec["code"]:
            return
        if got is not None:
            self.check_frames(got, rec, where)
        if rec["batch"]:
            frames, launches = c.batch_info()
            assert frames == n, f"trt_batch_info: {frames} frames of {n}\n{where}"
            expected = 1 <= launches <= n and (rec["launches"][0] != "equal" or launches == n)
            assert expected, f"{launches} render launches, the model expects {rec['launches']}\n{where}"
            if 1 < launches < n:
                self.split_launches.append((i, launches, n))
            assert launches > 1 or not splits_for_lds(rec), f"one render launch where the model expects LDS to split the batch\n{where}"
        self.last_render = (c, rec, where)
        if kind not in ("render_device", "render_device_batch"):
            self.check_counters()
        if rec["device_image"] is not None:
            in_device_memory = c.render_image()["in_device_memory"]
            assert in_device_memory == rec["device_image"], f"trt_render_image: the model expects in_device_memory = {rec['device_image']}\n{where}"


@gpu
@pytest.mark.parametrize("seed", SEEDS, ids=[f"seed{s}" for s in SEEDS])
def test_a_sequence_replayed_on_real_contexts(seed):
    ops = make_sequence(seed)
    replay = Replay(seed)
    try:
        for i in range(len(ops)):
            replay.step(i, ops)
        assert not replay.pending, "the generator ends every sequence with a synchronize"
    finally:
        replay.close_all()  # every context, whatever happened; each sequence has contexts of its own, so no default is left changed
    print(f"seed {seed}: {len(ops)} operations, {len(replay.oracle)} oracle frames, split batches (step, launches, n): {replay.split_launches}")
