"""The decoupled rounds' task ring, on the CPU: the oracle's ray log says what every sample of a directed launch does (tests/support.py,
oracle_hit_sequences), a model written from the kernel's stated rules says what a wave then does (tests/ring_model.py), and each launch of
tests/ring_cases.py is asserted to reach the state it is named for.  tests/test_decoupled_ring.py holds the device to the model's
rounds and passes and to the oracle's frames.  The last test asks whether the launches tell the rules from near misses of them."""
import numpy as np
import pytest

import ring_cases as RC
import ring_model as M
import support as T
import test_work_units as W


def test_the_launch_constants_are_the_sources():
    assert (RC.CHUNK, RC.CHUNK_SMALL, RC.XCD_SHIFT, RC.BLOCK, RC.COMPACT_BLOCK) == (W.CHUNK, W.CHUNK_SMALL, W.XCD_SHIFT, W.BLOCK, W.COMPACT_BLOCK)
    assert M.RING_TASKS == W._number(W._ROUNDS, r"kRingTasks = (\d+)") and M.LANES == M.PASS == 64
    for c in RC.CASES.values():  # the rings must fit: few spheres and lights; small frames, a workgroup's own chunks at the most
        assert c.scene.num_spheres <= 64 and len(c.scene.dir_lights) + len(c.scene.point_lights) == 2
        assert c.units <= (RC.COMPACT_BLOCK // 64) * RC.CHUNK and 1 <= c.spp <= 3


def test_hit_sequences_account_for_every_ray_of_the_oracle():
    """per unit in unit order: the rays add up to the frame's counts, the frame is the multi-threaded oracle's, the endings are the three
    kinds; a batch is frame-major"""
    for name in ("s6", "s7", "s10"):
        c, q = RC.CASES[name], RC.sequences(name)
        lights = len(c.scene.dir_lights) + len(c.scene.point_lights)
        assert q["paths"].shape == q["hits"].shape == q["ending"].shape == (c.units,)
        assert (int(q["paths"].sum()), int(q["hits"].sum()) * lights) == q["counts"]
        assert ((q["hits"] == q["paths"]) | (q["hits"] == q["paths"] - 1)).all()
        assert ((q["ending"] == T.ENDED_ON_SKY) == (q["hits"] < q["paths"])).all()
        assert ((q["ending"] == T.ENDED_BY_LIMIT) == (q["hits"] == c.bounce_limit)).all()
        assert all(len(r) == p for r, p in zip(q["rays"], q["paths"]))
        for k, cam in enumerate(c.cameras or [c.scene.camera]):
            want, st = T.oracle_render(c.scene.with_camera(cam), c.w, c.h, c.bounce_limit, c.spp)
            assert np.array_equal(T.bits(q["frames"][k]), T.bits(want))
    q = RC.sequences("s6")
    assert set(q["ending"].tolist()) == {T.ENDED_ON_SKY, T.ENDED_BY_LIMIT, T.ENDED_BY_WEIGHT}
    per = RC.CASES["s10"].w
    q = RC.sequences("s10")
    assert all(np.array_equal(q["paths"][:per], q["paths"][k * per:(k + 1) * per]) for k in range(3))  # three cameras, one pattern


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_the_models_hold_their_invariants_and_account_for_every_unit(name):
    """every wave of both models: each unit handed out exactly once, every colour of every sample added in bounce order, the sky's last"""
    c, q = RC.CASES[name], RC.sequences(name)
    for waves in (RC.decoupled(name), RC.plain(name)):
        handed = sorted(u for w in waves for u in w["lane_of"])
        assert handed == list(range(c.units))
    for w in RC.decoupled(name):
        for u, order in w["order"].items():
            want = tuple(range(q["hits"][u])) + ((M.SKY,) if q["hits"][u] < q["paths"][u] else ())
            assert order == want, (u, order, want)
        assert w["tasks"] == sum(int(q["hits"][u]) for u in w["lane_of"])
        assert w["occupancy"] <= 127 and max(w["carried"], default=0) <= 63


def test_without_a_hit_the_two_models_are_one():
    """300 units of sky in two waves: no task, no pass, the same rounds and the same lanes"""
    d, p = RC.decoupled("sky"), RC.plain("sky")
    assert len(d) == len(p) == 2 and RC.sequences("sky")["hits"].sum() == 0
    assert [w["rounds"] for w in d] == [w["rounds"] for w in p] == [4, 1]
    assert [w["lane_of"] for w in d] == [w["lane_of"] for w in p]
    assert RC.total(d, "passes") == RC.total(p, "passes") == 0


def one_wave(name):
    waves = RC.decoupled(name)
    assert len(waves) == 1
    return waves[0]


def test_s1_a_pass_of_64_from_an_empty_ring():
    w = one_wave("s1")
    assert w["new_tasks"] == [64] and w["carried"] == [0] and (w["rounds"], w["passes"]) == (1, 1)
    assert not w["waited"]  # the count alone triggered the pass: every colour arrived in its own round


def test_s2_63_carried_and_64_new_fill_the_ring_to_127():
    w = one_wave("s2")
    assert w["new_tasks"][:2] == [63, 64] and w["carried"][:2] == [63, 63] and w["occupancy"] == 127
    assert [r for r, _ in w["passes_of"]][0] == 2 and len(w["passes_of"][0][1]) == 64  # no pass in round 1; 64 of 127 in round 2
    assert w["carried_from"][1] == 64  # what is carried into round 3 is all of round 2: old by then
    assert (w["rounds"], w["passes"]) == (3, 2)


def test_s3_one_hit_per_round_wraps_the_ring_twice():
    """R5 as stated makes the passes of such a wave two tasks every other round (the task of the round before and this round's), not
    one task per round: a lone task is never old in the round it is made"""
    w = one_wave("s3")
    assert w["new_tasks"] == [1] * 300 and w["tasks"] == 300 > 2 * M.RING_TASKS + 1
    assert w["rounds"] == 300 and w["passes"] == 150 and all(len(units) == 2 for _, units in w["passes_of"])
    assert w["carried"] == [1, 0] * 150


def test_s4_a_carried_group_straddles_the_wrap():
    w = one_wave("s4")
    groups = [(first, n) for first, n in zip(w["carried_from"], w["carried"]) if n]
    assert (120, 16) in groups  # tasks 120 .. 135: slots 120 .. 127 and 0 .. 7
    assert {t % M.RING_TASKS for t in range(120, 136)} == set(range(120, 128)) | set(range(8))


@pytest.mark.parametrize("name", ["s5", "s5_limit", "s2"])
def test_s5_a_round_of_waiting_lanes_only(name):
    """the last round: nobody alive, the pool empty, every surviving lane waiting -- by weight, by the bounce limit, after two hits"""
    w = one_wave(name)
    last = w["rounds_of"][-1]
    assert last and all(what == "waited" for _, what in last.values()) and w["new_tasks"][-1] == 0
    assert len(last) == {"s5": 63, "s5_limit": 63, "s2": 63}[name]
    assert max(w["lane_of"]) == RC.CASES[name].units - 1  # nothing left to hand out
    ending = RC.sequences(name)["ending"]
    assert {int(ending[u]) for u, _ in last.values()} == {"s5": {T.ENDED_BY_WEIGHT}, "s5_limit": {T.ENDED_BY_LIMIT}, "s2": {T.ENDED_BY_WEIGHT}}[name]
    assert w["passes_of"][-1][0] == w["rounds"]  # ... and the pass that round runs for them


def test_s6_every_ending_in_one_round():
    w, ending = one_wave("s6"), RC.sequences("s6")["ending"]
    second = w["rounds_of"][1]
    kinds = {(what, int(ending[u]) if what in ("finished", "waits") else None) for u, what in second.values()}
    assert kinds == {("sky", None), ("continues", None), ("finished", T.ENDED_BY_LIMIT), ("waits", T.ENDED_BY_LIMIT), ("waits", T.ENDED_BY_WEIGHT)}
    assert len(second) == 64 and w["carried"][0] == 40 and w["new_tasks"][1] == 48  # 40 old and 48 new: the pass reaches 24 of the new


def hit_colours(name, unit):
    """what each hit of a unit adds to its sample: the lit colour times the weight the path has there"""
    c, q = RC.CASES[name], RC.sequences(name)
    probe = T.oracle_probe(c.scene, q["rays"][unit])
    weight = np.concatenate([[1.0], np.cumprod(probe["material"][:, 3])])[: len(probe["lit"])]
    return (probe["lit"] * weight[:, None])[: q["hits"][unit]]


def test_s7_two_colours_arrive_together_at_a_sample_that_is_not_zero():
    w = one_wave("s7")
    lanes, orders_differ = 0, 0
    for rnd, lane, unit in w["doubles"]:
        assert rnd == 3 and w["order"][unit][:3] == (0, 1, 2)
        s, a, b = hit_colours("s7", unit)[:3]
        if s.any() and len({tuple(T.bits(x).tolist()) for x in (s, a, b)}) == 3:
            lanes += 1
            orders_differ += not np.array_equal(T.bits((s + a) + b), T.bits((s + b) + a))
    assert lanes >= 16 and orders_differ >= 1, (lanes, orders_differ)


@pytest.mark.parametrize("name", ["s4"])
def test_s8_a_waiting_lane_changes_who_gets_which_unit(name):
    d, p = one_wave(name), RC.plain(name)[0]
    assert d["waited"] and d["lane_of"] != p["lane_of"] and sorted(d["lane_of"]) == sorted(p["lane_of"])


def test_s9_all_sixteen_rings_of_a_workgroup_hold_more_than_64():
    c, waves = RC.CASES["s9"], RC.decoupled("s9")
    grid, chunk = RC.launch_shape(c.units, RC.COMPACT_BLOCK)
    # one queue word: wave k of workgroup g owns chunk 16 g + k, so the sixteen chunks of the launch are workgroup 0's
    assert (grid, chunk) == (4, RC.CHUNK) and c.units == 16 * chunk and len(waves) == RC.COMPACT_BLOCK // 64 == 16
    assert all(w["occupancy"] > 64 for w in waves) and {w["occupancy"] for w in waves} == {127}


def test_s10_one_pass_shades_tasks_of_two_frames():
    c, w = RC.CASES["s10"], one_wave("s10")
    per = c.w * c.h * c.spp
    assert c.frames == 3 and per % 64 and w["occupancy"] == 127
    assert any(len({u // per for u in units}) > 1 for _, units in w["passes_of"])


MUTANTS = {
    "a ring of 64 slots": (M.RULES._replace(ring_tasks=64), "s2"),
    "a ring of 126 slots": (M.RULES._replace(ring_tasks=126), "s2"),
    "a pass only when more than 64 wait": (M.RULES._replace(pass_at=65), "s1"),
    "no pass for an old task": (M.RULES._replace(old_rule=False), "s5"),
    "no waiting round": (M.RULES._replace(wait_rounds=0), "s5"),
    "a wait of two rounds": (M.RULES._replace(wait_rounds=2), "s5"),
    "this round's colour before last round's": (M.RULES._replace(old_colour_first=False), "s7"),
}


def told_apart(name, rules):
    """does the launch tell `rules` from the stated ones: an invariant breaks, or rounds, passes or a sample's collection order change"""
    try:
        got = RC.decoupled(name, rules)
    except M.RingViolation as e:
        return str(e)
    want = RC.decoupled(name)
    for key in ("rounds", "passes", "order"):
        if [w[key] for w in got] != [w[key] for w in want]:
            return key
    return None


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_the_launches_tell_the_rules_from_near_misses(mutant):
    """Stands in for mutating the kernel.  What catches which:
      a ring of 64 slots, of 126 slots      s2: task 64 (126) is written over task 0, which no pass has shaded yet
      a pass only when more than 64 wait    s1: 64 tasks are carried over, and the launch takes two rounds
      no pass for an old task               s5: the waiting round finds last round's tasks unshaded
      no waiting round                      s5: the samples finish without their colour
      a wait of two rounds                  s5: three rounds for two
      this round's colour first             s7: the third hit's colour is added before the second's (s2: the second before the first,
                                            into a sample that is still zero -- which arithmetic cannot see)"""
    rules, name = MUTANTS[mutant]
    assert told_apart(name, rules), (mutant, name)
    assert not told_apart(name, M.RULES)
    caught_by = [n for n in sorted(RC.CASES) if told_apart(n, rules)]
    print(mutant, "is caught by", caught_by)
    assert name in caught_by
