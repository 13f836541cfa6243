"""A model of what ONE wave of the render rounds does with the work units it owns: plain Python, no device, written from the rules the
kernels' comments state (csrc/trt_rounds.hpp, COMPACT), not from their code.

A sample is all the model knows of a work unit: `paths` path rays of which the first `hits` meet a surface (tests/support.py,
oracle_hit_sequences).  A wave owns a run of units -- its own first chunk, cut by the end of the launch; what the queue would hand out
behind that lies behind the launch's end and holds nothing -- and the rules say what its 64 lanes do with them:

 R1 at the top of a round every lane that wants a unit gets the next one of the wave's pool, in lane order; a lane whose unit lies behind
    the end is dead;
 R2 the loop ends when no lane is alive and no lane waits; a round counts only if it gets past that test;
 R3 every alive lane traces one path ray per round;
 R4 a hit appends one task, in lane order, behind the tasks already in the ring;
 R5 after the hits are appended at most one pass runs: min(64, waiting tasks) from the head, if a task of an earlier round is among them
    or at least 64 wait;
 R6 a lane adds the colour of its previous round's task (always shaded by now), then this round's if the pass reached it, then the sky's
    if its ray left the scene;
 R7 a sample that ends on a hit whose colour has not arrived sits out exactly the next round, finishes at that round's end and only then
    wants a unit; every other ending wants a unit at once.

`Rules` holds the constants of R4, R5, R6 and R7, so that a test can ask whether a directed launch tells the stated rules from near
misses of them (tests/test_ring_model.py); the defaults are the rules.  plain_wave is the same hand-out without a ring: a finished lane
wants a unit at once, and every round with a hit has a pass."""
import collections

LANES = 64
PASS = 64           # tasks a pass shades at most: one per lane
RING_TASKS = 128    # kRingTasks
SKY = -1            # in a sample's collection order: the sky's colour (hits are numbered from 0)


class RingViolation(AssertionError):
    """an invariant that the rules imply does not hold"""


Rules = collections.namedtuple("Rules", "ring_tasks pass_at old_rule wait_rounds old_colour_first")
RULES = Rules(ring_tasks=RING_TASKS, pass_at=PASS, old_rule=True, wait_rounds=1, old_colour_first=True)

WANTS, ALIVE, WAITS, DEAD = "wants", "alive", "waits", "dead"


class _Lane:
    def __init__(self):
        self.state, self.unit, self.traced, self.wait_left = WANTS, None, 0, 0
        self.open = []       # tasks of this lane's sample whose colour it has not collected, oldest first
        self.collected = []  # the sample's colours in the order they were added: hit numbers, then SKY


class _Task:
    def __init__(self, number, lane, unit, hit, born):
        self.number, self.lane, self.unit, self.hit, self.born = number, lane, unit, hit, born
        self.shaded = self.collected = False


def _check(ok, *what):
    if not ok:
        raise RingViolation(what)


def _hand_out(lanes, pool, handed):
    """R1"""
    for i, lane in enumerate(lanes):
        if lane.state == WANTS:
            if pool:
                lane.state, lane.unit, lane.traced, lane.open, lane.collected = ALIVE, pool.popleft(), 0, [], []
                handed[lane.unit] = i
            else:
                lane.state = DEAD


def decoupled_wave(units, paths, hits, rules=RULES):
    """one wave of the decoupled rounds over `units` (an iterable of unit numbers, in order); paths[u], hits[u] describe unit u.
    Returns a dict: rounds, passes, occupancy (the highest), carried (after every round: how many tasks, carried_from: the number of the
    first of them), new_tasks (per round), tasks (how many were numbered), lane_of
    (unit -> lane), order (unit -> the order its colours were added in), doubles ([(round, lane, unit)]: two hit colours added in one
    round to a sample that held one already), waited ([(round, lane, unit)]: sat that round out), passes_of ([(round, [units of the
    tasks])]), rounds_of ([{lane: (unit, what)}]: per round and lane "sky", "finished", "waits" or "continues"; "waited" in the round a
    lane sits out)."""
    pool = collections.deque(units)
    lanes = [_Lane() for _ in range(LANES)]
    ring, tasks = {}, []                 # slot -> task; every task by number
    head = 0                             # tasks below it have been shaded
    out = {"rounds": 0, "passes": 0, "occupancy": 0, "carried": [], "carried_from": [], "new_tasks": [], "lane_of": {}, "order": {}, "doubles": [],
           "waited": [], "passes_of": [], "rounds_of": []}

    def finish(lane):
        _check(not lane.open, "a sample finished while a colour of its was outstanding", lane.unit)
        out["order"][lane.unit] = tuple(lane.collected)
        lane.state = WANTS

    while True:
        _hand_out(lanes, pool, out["lane_of"])
        if not any(l.state in (ALIVE, WAITS) for l in lanes):  # R2
            break
        out["rounds"] += 1
        now = out["rounds"]
        record = {}
        ended_on_hit, met_sky = set(), set()
        for i, lane in enumerate(lanes):  # R3, R4
            if lane.state != ALIVE:
                continue
            u = lane.unit
            if lane.traced < hits[u]:
                task = _Task(len(tasks), i, u, lane.traced, now)
                slot = task.number % rules.ring_tasks
                if slot in ring:
                    _check(ring[slot].shaded, "a task overwrote one that had not been shaded", task.number, ring[slot].number)
                    _check(ring[slot].collected, "a task overwrote a colour that had not been collected", task.number, ring[slot].number)
                ring[slot] = task
                tasks.append(task)
                lane.open.append(task)
                _check(len(lane.open) <= 2, "more than two colours outstanding", i, u)
            else:
                met_sky.add(i)
            lane.traced += 1
            if lane.traced == paths[u] and i not in met_sky:
                ended_on_hit.add(i)
        out["new_tasks"].append(sum(t.born == now for t in tasks[head:]))
        waiting = len(tasks) - head
        out["occupancy"] = max(out["occupancy"], waiting)
        _check(waiting <= RING_TASKS - 1, "more tasks wait than 63 carried over and 64 new", waiting)
        old = any(t.born < now for t in tasks[head:])
        if waiting and ((rules.old_rule and old) or waiting >= rules.pass_at):  # R5
            take = min(PASS, waiting)
            for t in tasks[head:head + take]:
                t.shaded = True
            out["passes"] += 1
            out["passes_of"].append((now, [t.unit for t in tasks[head:head + take]]))
            head += take
            _check(all(t.born == now for t in tasks[head:]), "a task of an earlier round survived a pass")
        out["carried"].append(len(tasks) - head)
        out["carried_from"].append(head)
        _check(len(tasks) - head <= PASS - 1, "more than 63 tasks carried over", len(tasks) - head)
        for i, lane in enumerate(lanes):  # R6, R7
            if lane.state not in (ALIVE, WAITS):
                continue
            before = len(lane.collected)
            mine = [t for t in lane.open if t.born == now]
            earlier = [t for t in lane.open if t.born < now]
            if not (lane.state == WAITS and lane.wait_left > 1):
                for t in earlier:
                    _check(t.born == now - 1 or rules.wait_rounds != 1, "a colour older than the previous round's was outstanding", i, t.number)
                    _check(t.shaded, "last round's task has not been shaded", i, t.number)
            arrived = [t for t in (earlier + mine if rules.old_colour_first else mine + earlier) if t.shaded]
            for t in arrived:
                t.collected = True
                lane.collected.append(t.hit)
                lane.open.remove(t)
            if len(arrived) == 2 and before >= 1:
                out["doubles"].append((now, i, lane.unit))
            if i in met_sky:
                lane.collected.append(SKY)
            if lane.state == WAITS:
                out["waited"].append((now, i, lane.unit))
                record[i] = (lane.unit, "waited")
                lane.wait_left -= 1
                if lane.wait_left == 0:
                    finish(lane)
            elif i in met_sky:
                record[i] = (lane.unit, "sky")
                finish(lane)
            elif i in ended_on_hit:
                if lane.open and rules.wait_rounds > 0:
                    record[i] = (lane.unit, "waits")
                    lane.state, lane.wait_left = WAITS, rules.wait_rounds
                else:
                    record[i] = (lane.unit, "finished")
                    finish(lane)
            else:
                record[i] = (lane.unit, "continues")
        out["rounds_of"].append(record)
    _check(head == len(tasks), "tasks were left unshaded", len(tasks) - head)
    out["tasks"] = len(tasks)
    return out


def plain_wave(units, paths, hits):
    """one wave of the plain rounds: R1 to R3; a lane shades its own hit in the round it finds it, so every round with a hit has a pass
    and a sample that ends wants a unit at once.  Returns rounds, passes, lane_of."""
    pool = collections.deque(units)
    lanes = [_Lane() for _ in range(LANES)]
    out = {"rounds": 0, "passes": 0, "lane_of": {}}
    while True:
        _hand_out(lanes, pool, out["lane_of"])
        alive = [l for l in lanes if l.state == ALIVE]
        if not alive:
            break
        out["rounds"] += 1
        out["passes"] += any(l.traced < hits[l.unit] for l in alive)
        for lane in alive:
            lane.traced += 1
            if lane.traced == paths[lane.unit]:
                lane.state = WANTS
    return out


def own_chunks(units, chunk, waves):
    """the runs of units that the waves of a launch own: chunk c is some wave's first as long as there are no more chunks than waves
    (every other chunk the queue hands out lies behind the launch's end)"""
    chunks = (units + chunk - 1) // chunk
    assert chunks <= waves, (units, chunk, waves)
    return [range(c * chunk, min((c + 1) * chunk, units)) for c in range(chunks)]


def launch(wave_model, units, chunk, waves, paths, hits, **more):
    """every wave of a launch that owns units: the waves' results in chunk order"""
    return [wave_model(run, paths, hits, **more) for run in own_chunks(units, chunk, waves)]
