"""The decoupled rounds' task ring on the device, steered through its edge states: the directed launches of tests/ring_cases.py, each of
which tests/test_ring_model.py shows to reach the state it is named for.  The scratch fill is on (tests/test_work_units.py): every frame
must be the oracle's bit for bit -- twice in a row and once straight after the plain kernel rendered the same frame -- and the counting
forms must count the oracle's rays, the model's rounds (wave_loop_trips) and the model's passes (shading_passes), the plain kernel
against the plain model.  Equalities throughout: the schedule of such a launch is fully determined."""
import numpy as np
import pytest

import ring_cases as RC
import test_work_units as W
from terminalraytracer_amd import hip

gpu = pytest.mark.gpu
SINGLE = sorted(n for n, c in RC.CASES.items() if c.cameras is None)
BATCH = sorted(n for n, c in RC.CASES.items() if c.cameras is not None)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    c.scene_name = None
    try:
        c.set_scratch_fill(True)
        yield c
    finally:
        c.enable_counters(False)
        c.set_compaction(-1)
        c.set_scene_image(-1)
        c.set_scratch_fill(False)
        c.close()


def configure(ctx, case, decoupled, count=False):
    ctx.set_kernel(hip.Context.PRODUCTION)
    ctx.set_compaction(1 if decoupled else 0)
    ctx.set_scene_image(0)
    ctx.enable_counters(count)
    if ctx.scene_name != case.name:
        ctx.set_scene(case.scene)
        ctx.scene_name = case.name


def ran(ctx, decoupled):
    v = ctx.render_variant()
    assert v == {"decoupled": decoupled, "workgroup_threads": RC.COMPACT_BLOCK if decoupled else RC.BLOCK}, v
    assert not ctx.render_image()["in_device_memory"] and ctx.path_patches()[0] == 0


def owns_every_chunk(ctx, case, decoupled):
    """the launch as the library planned it is the launch the model was given: not capped, the model's chunk size, and no more chunks
    than waves -- so every chunk inside the launch is some wave's own and none comes from the queue"""
    variant = "decoupled" if decoupled else "plain"
    p = W.plan(ctx, case.units, variant)
    grid, chunk = RC.launch_shape(case.units, W.block_of(variant))
    assert p["grid"] == p["want"] == grid < p["cap"] and p["chunk"] == chunk and p["words"] == (1 if grid < 1 << RC.XCD_SHIFT else 1 << RC.XCD_SHIFT), p
    assert (case.units + chunk - 1) // chunk <= grid * (p["block"] // 64), p
    return p


def render_once(ctx, case, decoupled, count=False):
    """one launch: the kernel asked for ran, the frames are the oracle's; a counting form counts the oracle's rays and the model's rounds
    and passes"""
    q = RC.sequences(case.name)
    configure(ctx, case, decoupled, count)
    rows = hip.RowSet.whole(case.w, case.h)
    if case.cameras is None:
        got = [ctx.render_host(case.scene.camera, rows, case.bounce_limit, case.spp)]
    else:
        got = ctx.render_host_batch(np.array(case.cameras), rows, case.bounce_limit, case.spp)
        assert ctx.batch_info() == (case.frames, 1)
    ran(ctx, decoupled)
    owns_every_chunk(ctx, case, decoupled)
    who = f"{case.name} {'decoupled' if decoupled else 'plain'}{' counting' if count else ''}"
    for k, want in enumerate(q["frames"]):
        W.same(got[k], want, f"{who}, frame {k}")
    if count:
        model = RC.decoupled(case.name) if decoupled else RC.plain(case.name)
        rays = ctx.read_counters()  # ... which also fetches what read_diagnostics reports
        diag = ctx.read_diagnostics()
        print(f"{who}: rays {rays} (oracle {q['counts']}), rounds {diag['wave_loop_trips']} (model {RC.total(model, 'rounds')}), "
              f"passes {diag['shading_passes']} (model {RC.total(model, 'passes')})")
        assert rays == q["counts"], who
        assert diag["wave_loop_trips"] == RC.total(model, "rounds"), who
        assert diag["shading_passes"] == RC.total(model, "passes"), who


@gpu
@pytest.mark.parametrize("name", SINGLE)
def test_a_directed_launch_is_the_oracles_frame_in_the_models_rounds_and_passes(ctx, name):
    """the states S1 to S9 (tests/test_ring_model.py says which launch reaches which) and the launch without a hit"""
    case = RC.CASES[name]
    render_once(ctx, case, True, count=True)
    render_once(ctx, case, True)
    render_once(ctx, case, True)
    render_once(ctx, case, False)
    render_once(ctx, case, True)
    render_once(ctx, case, False, count=True)
    render_once(ctx, case, True, count=True)


@gpu
@pytest.mark.parametrize("name", BATCH)
def test_a_directed_batch_is_the_oracles_frames(ctx, name):
    """S10: the batch form, whose lanes hold tasks of different frames in one pass.  There is no counting instantiation of a batch
    (csrc/trt_rounds.hpp: BATCH excludes COUNT), so its rounds and passes are the model's word alone; the same launch frame by frame
    is held to the model by the test above (s2)."""
    case = RC.CASES[name]
    render_once(ctx, case, True)
    render_once(ctx, case, True)
    render_once(ctx, case, False)
    render_once(ctx, case, True)
