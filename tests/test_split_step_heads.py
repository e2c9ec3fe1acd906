"""The split plan step -- walk, obstacle kernel, selection kernel -- with the step header in the leading (preloaded) arguments of the
obstacle and selection kernels (csrc/fx_obstacle_kernel.h ObstHead, fx_select.h SelectHead), the walk's per-candidate outputs
stored write-through (fx_split_wt) and no arg-min in the deferred walk, against the CPU oracle.  The decomposition of the
50 388-candidate step is forced on small grids: two lanes per candidate on the wave-split grid kernel (fx_set_tuning), the
obstacle stage as its own kernel at three steps per item (fx_set_obstacle_stage).

The grid is 3 x 5 x 9 = 135 candidates: three 64-entry tiles of the obstacle kernel with a ragged last one, two workgroups of the
walk, and five candidates per selection slice, so that the collision count is the sum of many slices' words.  Under the production
flag set 29 of the 135 are costed (the list fills half a tile, two tiles find nothing); with the debug flag set every candidate is
costed and the list fills the three tiles, 64 + 64 + 7."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import synthetic
from tests.test_hip_parity import RESULT_KEYS, _walled_in, compare, hip_hulls

pytestmark = pytest.mark.gpu

GRID = (3, 5, 8)   # (the current lateral offset joins the eight sampled ones)
MAIN = dict(ref_kind="arc", v0=10.0, grid=GRID, n_obstacles=3, lead_gap=20.0)   # obstacle 0: a slow lead vehicle on the reference line
WALL = dict(ref_kind="straight", v0=8.0, grid=GRID)
INFEASIBLE = dict(ref_kind="arc", kappa=0.05, v0=40.0, v_des=40.0, grid=GRID, n_obstacles=3)


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=4096, max_steps=30, max_ref_knots=1024, max_obstacles=64, max_pred_steps=64, max_agents=4)
    e.set_tuning(2, 2, 2, 0, 2)   # two lanes per candidate, two waves per SIMD, grid kernel, wave split
    e.set_obstacle_stage(2, 3)
    yield e
    e.close()


def is_split(eng, agents=1):
    info = eng.step_info()
    assert info["grid_kernel"] == 1 and info["lanes_per_candidate"] == 2 and info["wave_split"] == 1, info
    assert info["obstacle_kernel"] == 1 and info["obstacle_steps_per_item"] == 3 and info["obstacle_workgroup_waves"] == 10, info
    assert not info["fused_selection"] and not info["step_kernel"] and info["agents"] == agents, info


@pytest.fixture(scope="module")
def scenes():
    """name -> (inputs, the oracle's inputs, the oracle's answer), computed once"""
    from oracle import oracle
    out = {}
    for name, kw in (("main", MAIN), ("wall", WALL), ("infeasible", INFEASIBLE), ("k43", dict(MAIN, n_obstacles=43)),
                     ("second", dict(MAIN, seed=11, v0=8.0, lead_gap=15.0)), ("debug", dict(MAIN, draw_traj_set=True, kinematic_debug=True))):
        if name == "wall":
            inp, ref_inp = _walled_in(hip_hulls(), **kw), _walled_in(oracle.build_obstacle_hulls, **kw)
        else:
            inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
            ref_inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
        assert inp.n_candidates == 135
        out[name] = (inp, ref_inp, oracle.plan_step(ref_inp))
    return out


def check(eng, scene, res, agent=0):
    inp, ref_inp, want = scene
    compare(eng, inp, want, res, ref_inp=ref_inp, agent=agent)


def test_main_split_step_case(eng, scenes):
    """colliders ordered in front of the winner (the lead vehicle stands where the cheapest candidates go): counted by many slices"""
    want = scenes["main"][2]
    assert want["result"]["best_index"] >= 0 and want["result"]["n_collisions"] > 0
    res = eng.plan_step(scenes["main"][0])
    is_split(eng)
    check(eng, scenes["main"], res)
    assert res["n_collisions"] == want["result"]["n_collisions"] and res["best_index"] == want["result"]["best_index"]


def test_main_case_with_every_candidate_listed(eng, scenes):
    """the debug flag set: all 135 candidates are costed -- three tiles of the list, the last one ragged"""
    want = scenes["debug"][2]
    assert int(want["costed"].sum()) == 135 and want["result"]["n_collisions"] > 0
    res = eng.plan_step(scenes["debug"][0])
    is_split(eng)
    check(eng, scenes["debug"], res)
    assert res["n_collisions"] == want["result"]["n_collisions"] and res["best_index"] == want["result"]["best_index"]


def test_nothing_collision_free(eng, scenes):
    want = scenes["wall"][2]
    assert want["result"]["best_index"] == -1 and want["result"]["n_collisions"] == int(want["selectable"].sum()) > 16
    res = eng.plan_step(scenes["wall"][0])
    is_split(eng)
    check(eng, scenes["wall"], res)
    assert res["best_index"] == -1 and res["n_collisions"] == want["result"]["n_collisions"]


def test_empty_list(eng, scenes):
    want = scenes["infeasible"][2]
    assert int(want["costed"].sum()) == 0
    res = eng.plan_step(scenes["infeasible"][0])
    is_split(eng)
    check(eng, scenes["infeasible"], res)
    assert res["best_index"] == -1 and res["n_collisions"] == 0 and res["n_feasible"] == 0


def test_second_table_round(eng, scenes):
    """43 obstacles x 3 steps = 129 (step, obstacle) entries per item: one more than the two the lanes stage at entry"""
    res = eng.plan_step(scenes["k43"][0])
    is_split(eng)
    check(eng, scenes["k43"], res)


def test_batch_between_single_agent_steps(eng, scenes):
    """a batch of two agents (no step header: every workgroup reads its agent's problem) between single-agent steps on one context"""
    pair = [scenes["main"], scenes["second"]]
    for _ in range(2):
        res = eng.plan_step(scenes["main"][0])
        is_split(eng)
        check(eng, scenes["main"], res)
        eng.upload([s[0] for s in pair])
        eng.evaluate()
        both = eng.finish()
        is_split(eng, agents=2)
        for a, s in enumerate(pair):
            check(eng, s, both[a], agent=a)
        res = eng.plan_step(scenes["second"][0])
        is_split(eng)
        check(eng, scenes["second"], res)


def test_two_hundred_steps_on_one_context(eng, scenes):
    """alternating inputs, uploaded and resident: no slice word, counter or list length of one step survives into the next"""
    order = ["main", "wall", "main", "infeasible", "second"]
    first = {}
    for name in order:
        first[name] = eng.plan_step(scenes[name][0])
        check(eng, scenes[name], first[name])
    assert len({first[n]["n_collisions"] for n in order}) >= 3   # the steps' collision counts differ: a stale word would show
    steps = 0
    while steps < 200:
        for name in order:
            res = eng.plan_step(scenes[name][0])
            assert {k: res[k] for k in RESULT_KEYS} == {k: first[name][k] for k in RESULT_KEYS}, (steps, name)
            eng.evaluate()   # the same inputs again, resident
            again = eng.finish()[0]
            assert {k: again[k] for k in RESULT_KEYS} == {k: first[name][k] for k in RESULT_KEYS}, (steps, name, "resident")
            steps += 2
    is_split(eng)
    check(eng, scenes["second"], res)
