"""The re-score pass (FrenetEngine.rescore, fx_rescore_agent) behind real plan steps: grid (8, 16, 16) (+ d0) = 2 176
candidates with 8 obstacles, the default five cost terms.

What it must answer is what a plan step run with the other weights stores: the same cost bits on every costed candidate and the same
winner -- in the summation form of a step whose obstacle stage ran inside the walk and in the form of a step whose obstacle kernel
closed the sum (FX_MODE_INT_DEFER_OBST); `step_info()` says which ran.  Nothing of the step is touched, any agent of a batch context
answers as it does alone, and every refusal leaves the context as it was."""
import ctypes as C

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
from tests import device_planes as dp

pytestmark = pytest.mark.gpu

GRID = (8, 16, 16)
COSTED = _abi.FX_FLAG_COSTED
NAMES = sorted(DEFAULT_COST_WEIGHTS)


def make(grid=GRID, n_obstacles=8, **kw):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=grid, n_obstacles=n_obstacles, **kw)


def engine(inp, stage=0, **kw):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=inp.n_candidates_global, device=0, **kw)
    if stage:
        e.set_obstacle_stage(stage)
    return e


def weight_sets():
    """the step's own weights; all of them scaled; permuted among the terms (twice); one with a negative weight"""
    d = dict(DEFAULT_COST_WEIGHTS)
    vals = [d[n] for n in NAMES]
    return [d, {n: 3.7 * d[n] for n in NAMES}, dict(zip(NAMES, vals[1:] + vals[:1])), dict(zip(NAMES, vals[::-1])),
            dict(d, lateral_jerk=-0.05, velocity_offset=2.5)]


def local_winner(inp, res):
    return res["best_index"] - inp.shard_begin if res["best_index"] >= 0 else -1


@pytest.mark.parametrize("shard", (None, (300, 1500)))
def test_the_steps_own_weights_reproduce_the_step(shard):
    inp = make()
    inp.shard = shard
    assert inp.cost_names == NAMES and inp.n_candidates == (1500 if shard else 2176)
    with engine(inp) as e:
        res = e.plan_step(inp)
        cost, flags = e.costs()
        W = np.array([inp._cost_w, 2.0 * inp._cost_w])
        r = e.rescore(W, totals=True)
        costed = (flags & COSTED) != 0
        assert 100 < costed.sum() < inp.n_candidates and res["best_index"] >= 0
        assert r["totals"].shape == (2, inp.n_candidates)
        assert np.array_equal(dp.bits(r["totals"][0][costed]), dp.bits(cost[costed])) and np.all(np.isnan(r["totals"][:, ~costed]))
        assert r["winner"][0] == local_winner(inp, res) and dp.bits(r["cost"][0]) == dp.bits(res["best_cost"])
        assert 0 <= r["winner"][0] < inp.n_candidates and dp.bits(r["cost"][0]) == dp.bits(cost[r["winner"][0]])
        assert e.last_rescore_ms > 0.0
        # the same through name -> weight dicts, and without the totals
        r2 = e.rescore([dict(zip(NAMES, w)) for w in W])
        assert r2["totals"] is None and np.array_equal(r2["winner"], r["winner"]) and np.array_equal(dp.bits(r2["cost"]), dp.bits(r["cost"]))


@pytest.mark.parametrize("stage", (0, 1, 2))
def test_other_weights_equal_a_real_step_run_with_them(stage):
    """stage 0: as the policy chooses at this size; 1: the obstacle stage inside the walk (the undeferred sum); 2: its own kernel,
    which closes the sum (the deferred form)"""
    sets = weight_sets()
    inp = make()
    with engine(inp, stage) as e, engine(inp, stage) as e2:
        e.plan_step(inp)
        form = e.step_info()["obstacle_kernel"]
        assert stage == 0 or form == (stage == 2)
        r = e.rescore(sets, totals=True)
        assert r["totals"].shape == (len(sets), inp.n_candidates)
        for k, d in enumerate(sets):
            other = make(cost_weights=d)
            assert other.cost_names == NAMES
            res = e2.plan_step(other)
            assert e2.step_info()["obstacle_kernel"] == form               # the same form really ran
            cost, flags = e2.costs()
            costed = (flags & COSTED) != 0
            assert costed.sum() > 100
            assert np.array_equal(dp.bits(r["totals"][k][costed]), dp.bits(cost[costed])), (stage, k)
            assert np.all(np.isnan(r["totals"][k][~costed]))
            assert r["winner"][k] == res["best_index"] and dp.bits(r["cost"][k]) == dp.bits(res["best_cost"]), (stage, k)


def test_nothing_of_the_step_is_touched():
    inp = make()
    with engine(inp) as e:
        res = e.plan_step(inp)

        def state():
            cost, flags = e.costs()
            tc, ti = e.topk(16)
            return dp.bits(cost), flags, dp.bits(e.costmap()), dp.bits(tc), ti, dp.bits(e.plane("x"))

        before = state()
        sets = weight_sets()
        e.rescore(sets, totals=True)
        e.rescore(np.array([[1.0, -2.0, 3.0, 0.5, 0.25]] * 70), totals=True)       # (the vector regime)
        after = state()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert before[4][0][0] == res["best_index"]


def test_an_agent_of_a_batch_answers_as_it_does_alone():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inps = [make(grid=(5, 9, 11), n_obstacles=4), make(grid=GRID, n_obstacles=8, v_des=11.0), make(grid=(4, 8, 12), n_obstacles=2)]
    sizes = [i.n_candidates for i in inps]
    assert len(set(sizes)) == 3
    sets = weight_sets()
    with FrenetEngine(max_candidates=sum(sizes) + 64 * 3, max_agents=3) as eb, engine(inps[1]) as e1:
        results = eb.plan_batch(inps)
        e1.plan_step(inps[1])
        rb = eb.rescore(sets, agent=1, totals=True)
        r1 = e1.rescore(sets, totals=True)
        assert rb["totals"].shape == (len(sets), sizes[1])
        assert np.array_equal(rb["winner"], r1["winner"]) and np.array_equal(dp.bits(rb["cost"]), dp.bits(r1["cost"]))
        assert np.array_equal(np.isnan(rb["totals"]), np.isnan(r1["totals"]))
        ok = ~np.isnan(r1["totals"])
        assert np.array_equal(dp.bits(rb["totals"][ok]), dp.bits(r1["totals"][ok]))
        assert rb["winner"][0] == results[1]["best_index"]
        # the other agents answer too, each with its own candidate count
        for a in (0, 2):
            r = eb.rescore(sets[:2], agent=a, totals=True)
            assert r["totals"].shape == (2, sizes[a]) and r["winner"][0] == results[a]["best_index"]


def test_refusals_leave_the_context_as_it_was():
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = make()
    own = np.array([inp._cost_w])

    def raw_call(e, n_vec, w, winner=True, cost=True):
        win, c = np.zeros(max(n_vec, 1), np.int64), np.zeros(max(n_vec, 1))
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        return lib().fx_rescore_agent(e._ctx, 0, n_vec, None if w is None else ptr(w), ptr(win) if winner else None, ptr(c) if cost else None, None)

    # no step at all; a select-only step
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as e:
        with pytest.raises(ValueError):
            e.rescore(own)
        assert raw_call(e, 1, own) == _abi.FX_ERR_NOT_READY
        sel = make(write_bundle=False, write_costmap=False)
        e.plan_step(sel)
        with pytest.raises(ValueError, match="FX_MODE_WRITE_COSTMAP"):
            e.rescore(own)
        assert raw_call(e, 1, own) == _abi.FX_ERR_NOT_READY
        with pytest.raises(ValueError, match="FX_MODE_WRITE_COSTMAP"):
            e.costmap_view()
        res = e.plan_step(inp)                                     # and the same context answers behind a full step
        assert e.rescore(own)["winner"][0] == res["best_index"]
    with engine(inp) as e:
        res = e.plan_step(inp)
        good = e.rescore(own, totals=True)

        def still_answers():
            r = e.rescore(own, totals=True)
            assert r["winner"][0] == good["winner"][0] == res["best_index"] and rp_same(r["totals"], good["totals"])

        for bad in (0.0, -0.0, np.nan, np.inf, -np.inf):
            w = np.array([inp._cost_w, inp._cost_w])
            w[1, 3] = bad
            with pytest.raises(ValueError):
                e.rescore(w)
            assert raw_call(e, 2, w) == _abi.FX_ERR_INVALID_ARGUMENT       # (the library's own check, behind the wrapper's)
            still_answers()
        with pytest.raises(ValueError):
            e.rescore(np.zeros((0, len(NAMES))))
        assert raw_call(e, 0, own) == _abi.FX_ERR_INVALID_ARGUMENT and raw_call(e, -1, own) == _abi.FX_ERR_INVALID_ARGUMENT
        assert raw_call(e, 1, None) == raw_call(e, 1, own, winner=False) == raw_call(e, 1, own, cost=False) == _abi.FX_ERR_INVALID_ARGUMENT
        big = np.ones((_abi.FX_RESCORE_MAX_VECTORS + 1, len(NAMES)))
        assert raw_call(e, len(big), big) == _abi.FX_ERR_CAPACITY
        still_answers()
        with pytest.raises(ValueError):
            e.rescore(own, agent=1)
        for names in (dict(DEFAULT_COST_WEIGHTS, jerk=0.1), {n: 1.0 for n in NAMES[:-1]}, dict(DEFAULT_COST_WEIGHTS, prediction=0.0)):
            with pytest.raises(ValueError, match="not the step's"):
                e.rescore([names])
        assert e.rescore([dict(DEFAULT_COST_WEIGHTS, jerk=0.0)])["winner"][0] == res["best_index"]    # (a zero entry is no term)
        with pytest.raises(ValueError):
            e.rescore(np.ones((2, len(NAMES) + 1)))
        still_answers()
        # inputs rewritten since the evaluation: the rows are of a step that has not run
        e.update_state(e.make_state_update(v_des=inp.v_des + 1.0))
        with pytest.raises(ValueError, match="rewritten"):
            e.rescore(own)
        e.update_state(e.make_state_update(v_des=inp.v_des))
        e.evaluate()
        e.finish()
        still_answers()


def rp_same(a, b):
    from tests import rescore_planes as rp
    return rp.same_nan_or_bits(a, b)


def test_the_planner_rescoring_its_last_step():
    """ReactivePlannerHip.rescore on last_step: (index, cost) per weight set, the first being the step's own selection"""
    from tests.test_hip_planner import make_planner
    rp_, _ = make_planner()
    try:
        with pytest.raises(ValueError, match="no plan step"):
            rp_.rescore([dict(DEFAULT_COST_WEIGHTS)])
        assert rp_.plan() is not None
        step = rp_.last_step
        own = dict(zip(step.inputs.cost_names, step.inputs._cost_w))
        out = rp_.rescore([own, {n: 2.0 * w for n, w in own.items()}])
        assert len(out) == 2 and out[0][0] == out[1][0] == local_winner(step.inputs, step.result)
        assert dp.bits(out[0][1]) == dp.bits(step.result["best_cost"])
    finally:
        rp_.close()
