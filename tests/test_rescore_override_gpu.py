"""The re-score over effective cost lists behind REAL plan steps whose cost is partly summed beside the step:
grid (8, 16, 16) (+ d0) = 2 176 candidates with 4 obstacles, the collision-probability pass (section 16) as the prediction entry and
the responsibility pass (section 17) as one more term.

  * re-scoring with the step's own weights and the passes' rows reproduces the pass's `total` and `best`, bit for bit;
  * five other weight sets equal real steps run with those weights plus the same passes -- with the obstacle stage as the policy
    chooses, forced into the walk (the undeferred sum) and forced into its own kernel (the deferred sum, whose tail the inserted
    term joins);
  * ReactivePlannerHip.rescore(rows="override") and AgentBatchHip.rescore agree with the engine calls they are made of, touch
    nothing of any step, and refuse what they must before any call."""
import os

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import device_planes as dp
from tests import rescore_rows as rr

pytestmark = pytest.mark.gpu

COSTED = _abi.FX_FLAG_COSTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")


def weight_sets(names, own, w_resp):
    """name -> weight over the effective names: the step's own; all scaled; permuted among the terms (twice); a negative weight;
    another responsibility weight"""
    eff = list(names) + ["responsibility"]
    d = dict(zip(eff, list(own) + [w_resp]))
    vals = [d[n] for n in eff]
    return [d, {n: 3.7 * d[n] for n in eff}, dict(zip(eff, vals[1:] + vals[:1])), dict(zip(eff, vals[::-1])),
            dict(d, lateral_jerk=-0.05, velocity_offset=2.5), dict(d, responsibility=4.0 * w_resp)]


def passes(eng, inp, params, w_resp):
    """the obstacles, reach sets and action-space vector of tests/test_responsibility_cost_gpu.py on the step's own planes, then the
    responsibility pass with the collision probability as the prediction entry"""
    from tests.test_responsibility_cost_gpu import _cost, _planes, _setup
    _, flags = eng.costs()
    resp_vec = _setup(eng, inp, flags, _planes(eng))[4]
    return eng.responsibility_cost(params, _cost(resp_vec), w_resp, prediction="probability"), flags


@pytest.mark.parametrize("stage", (0, 1, 2))
def test_real_steps_with_both_passes(stage):
    from frenetix_motion_planner_amd import risk
    from tests.test_responsibility_cost_gpu import W_RESP, _engine, _make
    from tests.test_risk_gpu import BASE, EGO, HARM
    params = risk.risk_params(BASE, HARM, **EGO)
    inp = _make()
    names = list(inp.cost_names)
    sets = weight_sets(names, inp._cost_w, W_RESP)
    with _engine(inp) as e, _engine(inp) as e2:
        for x in (e, e2):
            if stage:
                x.set_obstacle_stage(stage)
        e.plan_step(inp)
        form = bool(e.step_info()["obstacle_kernel"])
        assert stage == 0 or form == (stage == 2)
        own, flags = passes(e, inp, params, W_RESP)
        costed = (flags & COSTED) != 0
        assert costed.sum() > 100 and own["best_index"] >= 0 and (own["resp"][costed] != 0).any()
        assert (own["prediction"][costed] != e.costmap()[costed, names.index("prediction")]).any()
        before = dp.bits(e.costs()[0]), dp.bits(e.costmap())
        r = e.rescore(sets, pred=own["prediction"], resp=own["resp"], totals=True)
        assert r["totals"].shape == (len(sets), inp.n_candidates) and np.all(np.isnan(r["totals"][:, ~costed]))
        # the step's own weights: the override's total and best
        assert np.array_equal(dp.bits(r["totals"][0][costed]), dp.bits(own["total"][costed]))
        assert r["winner"][0] == own["best_index"] and dp.bits(r["cost"][0]) == dp.bits(own["best_cost"])
        assert len({int(w) for w in r["winner"]}) > 1                    # (the sets do not all choose the same candidate)
        # the batch form of the same call, and the same through arrays
        rb = e.rescore_batch([sets], pred=[own["prediction"]], resp=[own["resp"]])[0]
        rr.same_result(rb, r["winner"], r["cost"], stage)
        eff = names[:names.index("prediction") + 1] + ["responsibility"] + names[names.index("prediction") + 1:]
        ra = e.rescore(np.array([[d[n] for n in eff] for d in sets]), pred=own["prediction"], resp=own["resp"])
        rr.same_result(ra, r["winner"], r["cost"], stage)
        after = dp.bits(e.costs()[0]), dp.bits(e.costmap())
        assert all(np.array_equal(a, b) for a, b in zip(before, after))  # nothing of the step is touched
        # five other sets: real steps run with those weights plus the same passes
        for k, d in enumerate(sets[1:], 1):
            other = _make(cost_weights={n: d[n] for n in names})
            assert list(other.cost_names) == names
            e2.plan_step(other)
            assert bool(e2.step_info()["obstacle_kernel"]) == form          # the same form really ran
            real, f2 = passes(e2, other, params, d["responsibility"])
            assert np.array_equal(f2, flags)
            assert np.array_equal(dp.bits(r["totals"][k][costed]), dp.bits(real["total"][costed])), (stage, k)
            assert r["winner"][k] == real["best_index"] and dp.bits(r["cost"][k]) == dp.bits(real["best_cost"]), (stage, k)


def _own_sets(step):
    own = dict(zip(step.inputs.cost_names, (float(w) for w in step.inputs._cost_w)))
    if "responsibility" in step._extras:
        own["responsibility"] = step._extras["responsibility"][1]
    return [own, {n: 2.0 * w for n, w in own.items()}, dict(own, prediction=3.0 * own["prediction"])]


def test_the_planner_rescoring_its_override():
    from tests.test_responsibility_planner import _planner
    rp = _planner("action_space", prediction_cost="collision_probability")
    try:
        with pytest.raises(ValueError, match="no plan step"):
            rp.rescore([{}], rows="override")
        assert rp.plan() is not None
        step = rp.last_step
        assert step._override is not None and "responsibility" in step._extras
        sets = _own_sets(step)
        cost_before = step.cost.copy()
        out = rp.rescore(sets, rows="override")
        pred, resp = rp.rescore_rows(step, "override")
        assert pred is not None and resp is not None
        want = step.engine.rescore(sets, agent=step.agent, pred=pred, resp=resp, totals=True)
        assert out == [(int(i), float(c)) for i, c in zip(want["winner"], want["cost"])]
        # the planner's own weights: the cost it ranks by and the candidate it chose
        costed = (step._flags & COSTED) != 0
        assert np.array_equal(dp.bits(want["totals"][0][costed]), dp.bits(step.cost[costed]))
        assert out[0][0] == step._override[2] and out[1][0] == out[0][0]
        assert np.array_equal(dp.bits(step.cost), dp.bits(cost_before)) and rp.last_step is step
        # the default is the step's own rows and the step's own names
        with pytest.raises(ValueError, match="not the step's"):
            rp.rescore(sets)
        plain = rp.rescore([{n: w for n, w in sets[0].items() if n != "responsibility"}])
        assert plain[0][0] == step.result["best_index"] - step.inputs.shard_begin and dp.bits(plain[0][1]) == dp.bits(step.result["best_cost"])
        with pytest.raises(ValueError, match="rows"):
            rp.rescore(sets, rows="passes")
        assert rp.rescore(sets, rows="override") == out                     # a refusal leaves everything usable
    finally:
        rp.close()


def test_a_step_without_an_override_is_refused():
    from tests.test_hip_planner import make_planner
    rp, _ = make_planner()
    try:
        assert rp.plan() is not None and rp.last_step._override is None
        own = dict(zip(rp.last_step.inputs.cost_names, rp.last_step.inputs._cost_w))
        with pytest.raises(ValueError, match="override"):
            rp.rescore([own], rows="override")
        assert rp.rescore([own])[0][0] == rp.last_step.result["best_index"]
    finally:
        rp.close()


@pytest.mark.parametrize("groups", (1, 2))
def test_the_agent_batch_rescoring_its_steps(groups):
    from frenetix_motion_planner_amd import commonroad_xml as crx, multiagent
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
    cfg = PlannerConfig(prediction_cost="collision_probability")
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=cfg, pipeline_groups=groups)
    try:
        batch = sim.batch
        with pytest.raises(ValueError, match=f"agent {batch.agents[0].id} has no current plan step"):
            batch.rescore({batch.agents[0].id: [{}]})
        sim.step()
        agents = [batch.agents[k] for k in (3, 0, 2)]                       # three agents, out of order, across the groups
        steps = {a.id: a.planner.last_step for a in agents}
        assert all(s is not None and s._override is not None for s in steps.values())
        assert len({id(s.engine) for s in steps.values()}) == groups
        sets = {a.id: _own_sets(steps[a.id])[: 1 + k] for k, a in enumerate(agents)}
        before = {i: dp.bits(s.cost).copy() for i, s in steps.items()}
        out = batch.rescore(sets, rows="override")
        assert list(out) == list(sets)
        for a in agents:
            step = steps[a.id]
            pred, resp = a.planner.rescore_rows(step, "override")
            assert pred is not None and resp is None
            want = step.engine.rescore(sets[a.id], agent=step.agent, pred=pred, totals=True)
            assert out[a.id] == [(int(i), float(c)) for i, c in zip(want["winner"], want["cost"])]
            costed = (step._flags & COSTED) != 0
            assert np.array_equal(dp.bits(want["totals"][0][costed]), dp.bits(step.cost[costed]))
            assert out[a.id][0][0] == step._override[2]
            assert a.planner.rescore(sets[a.id], rows="override") == out[a.id]
            assert np.array_equal(dp.bits(step.cost), before[a.id])
        # the step's own rows: the step's own selection
        plain = batch.rescore({a.id: sets[a.id][:1] for a in agents})
        for a in agents:
            step = steps[a.id]
            assert plain[a.id][0][0] == (step.result["best_index"] - step.inputs.shard_begin if step.result["best_index"] >= 0 else -1)
        # refused by name before any call: an agent that is not of the batch; a weight set that is not the step's
        with pytest.raises(ValueError, match="agent -5 is not of this batch"):
            batch.rescore({agents[0].id: sets[agents[0].id], -5: [{}]})
        with pytest.raises(ValueError):
            batch.rescore({agents[0].id: [dict(sets[agents[0].id][0], jerk=0.3)]}, rows="override")
        assert batch.rescore(sets, rows="override") == out
    finally:
        sim.close()
