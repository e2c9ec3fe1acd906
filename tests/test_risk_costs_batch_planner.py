"""AgentBatchHip(batched_risk_costs=...) on the HIP engine: the "min_risk_cost" fallbacks of blocked planners
(tests/test_planner_host.py: every feasible candidate collides) choose the same samples with the same risk bits whether they run
as ONE risk_costs_batch per engine group and planning step or as one risk_costs call per agent, in both responsibility modes and
beside the batched risk call of section 20; the calls are counted on an engine subclass."""
import os

import numpy as np
import pytest

from frenetix_motion_planner_amd import commonroad_xml as crx, engine as engine_module, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
from tests.test_risk_batch_planner import _Agent
from tests.test_risk_costs_planner import WEIGHTS, _reach_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")


class CountingEngine(engine_module.FrenetEngine):
    """the HIP engine with its risk entrances counted"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def risk(self, params, ids=None, agent=0):
        self.calls.append(("risk", int(agent), None if ids is None else len(ids)))
        return super().risk(params, ids, agent)

    def risk_batch(self, params, ids=None, agents=None):
        self.calls.append(("risk_batch", tuple(agents), tuple(None if x is None else len(x) for x in ids)))
        return super().risk_batch(params, ids, agents)

    def risk_costs(self, params, cost_params, ids=None, agent=0):
        self.calls.append(("risk_costs", int(agent), None if ids is None else len(ids)))
        return super().risk_costs(params, cost_params, ids, agent)

    def risk_costs_batch(self, params, cost_params, ids=None, agents=None):
        self.calls.append(("risk_costs_batch", tuple(agents), tuple(None if x is None else len(x) for x in ids)))
        return super().risk_costs_batch(params, cost_params, ids, agents)


def _planner(k, selector, mode=None, free=False, **cfg):
    from tests.test_planner_host import blocked_planner
    from tests.test_risk_planner import HARM, MASS, RISK
    rp = blocked_planner(engine=None, **cfg)
    wall = rp.predictions[5]
    wall["v_list"] = np.full(len(wall["pos_list"]), 0.5 + 0.25 * k)
    if free:   # the wall stands far beside the road
        wall["pos_list"] = wall["pos_list"] + np.array([0.0, 60.0])
    rp.set_predictions({5: wall})
    rp.set_risk_model(RISK, HARM, {5: "car"}, MASS)
    if selector == "min_risk_cost":
        rp.set_risk_cost_weights(WEIGHTS, responsibility_mode=mode)
        rp.set_reach_set(_reach_set(rp))
    if selector is not None:
        rp.set_fallback_selector(selector)
    return rp


def _step(planners, **flags):
    cap = max(4096, max(p.max_candidates_per_step() for p in planners))
    batch = multiagent.AgentBatchHip([_Agent(10 + k, p) for k, p in enumerate(planners)], max_candidates=cap, pipeline_groups=1, **flags)
    eng = batch.engine
    assert isinstance(eng, CountingEngine)
    try:
        batch.step(0, {})
        out = []
        for p in planners:
            best = p.optimal_trajectory
            out.append(None if best is None else (best.uniqueId, None if best._ego_risk is None else np.float64(best._ego_risk).tobytes(),
                                                  None if best._obst_risk is None else np.float64(best._obst_risk).tobytes()))
        pairs = [None if a.pair is None or p.optimal_trajectory is None else
                 b"".join(np.asarray(getattr(p.optimal_trajectory.cartesian, n), np.float64).tobytes() for n in ("x", "y", "theta", "v"))
                 for a, p in zip(batch.agents, planners)]
        own = [list(getattr(p._engine, "calls", [])) if p._engine is not None else [] for p in planners]
        return out, list(eng.calls), own, [p.last_step.result["best_index"] for p in planners], pairs
    finally:
        batch.close()


def test_min_risk_cost_fallbacks_in_both_modes(monkeypatch):
    """three blocked planners -- action-space, reach-set and no responsibility -- and a free one"""
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)

    def four():
        return [_planner(0, "min_risk_cost", "action_space"), _planner(1, "min_risk_cost", "reach_set"),
                _planner(2, "min_risk_cost", None, free=True), _planner(3, "min_risk_cost", None)]

    off = _step(four(), batched_risk_costs=False)
    on = _step(four(), batched_risk_costs=True)
    assert on[0] == off[0] and on[3] == off[3] and on[4] == off[4]
    assert [b == -1 for b in off[3]] == [True, True, False, True]
    # the blocked ones chose by risk cost and carry the risks; the free one chose by cost and carries none
    assert all(off[0][k] is not None and off[0][k][1] is not None and off[0][k][2] is not None for k in (0, 1, 3))
    assert off[0][2] is not None and off[0][2][1] is None and all(p is not None for p in off[4])
    assert any(np.frombuffer(off[0][k][1])[0] > 0 for k in (0, 1, 3)), "no chosen trajectory with a risk"
    # off: one per-agent call of each blocked planner over its feasible candidates; on: the ONE call, no per-agent one
    assert [c[:2] for c in off[1]] == [("risk_costs", 0), ("risk_costs", 1), ("risk_costs", 3)] and all(c[2] > 1 for c in off[1])
    assert on[1] == [("risk_costs_batch", (0, 1, 3), tuple(c[2] for c in off[1]))], on[1]
    assert not any(off[2]) and not any(on[2])


def test_mixed_batch(monkeypatch):
    """a "min_risk" planner, a "min_risk_cost" planner (both blocked) and a free log_risk planner: one risk_batch and one
    risk_costs_batch, the results of the per-agent path"""
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)

    def three():
        return [_planner(0, "min_risk"), _planner(1, "min_risk_cost", "action_space"), _planner(2, None, free=True, log_risk=True)]

    off = _step(three())
    on = _step(three(), batched_risk=True, batched_risk_costs=True)
    assert on[0] == off[0] and on[3] == off[3] and on[4] == off[4]
    assert off[3][0] == -1 and off[3][1] == -1 and off[3][2] >= 0
    assert all(c is not None and c[1] is not None for c in off[0])
    assert [c[:2] for c in off[1]] == [("risk", 0), ("risk_costs", 1), ("risk", 2)] and off[1][2][2] == 1
    assert sorted(on[1]) == [("risk_batch", (0, 2), (None, 1)), ("risk_costs_batch", (1,), (off[1][1][2],))], on[1]
    # either flag alone: the other kind keeps its per-agent call, the same results
    for flags, calls in ((dict(batched_risk=True), ["risk_batch", "risk_costs"]), (dict(batched_risk_costs=True), ["risk", "risk", "risk_costs_batch"])):
        one = _step(three(), **flags)
        assert one[0] == off[0] and one[4] == off[4] and sorted(c[0] for c in one[1]) == calls, (flags, one[1])


def test_an_escalating_planner_keeps_the_per_agent_path(monkeypatch):
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)

    def two():
        return [_planner(0, "min_risk_cost", "action_space", sampling_min=2, sampling_max=4), _planner(1, "min_risk_cost", "action_space")]

    off = _step(two(), batched_risk_costs=False)
    on = _step(two(), batched_risk_costs=True)
    assert on[0] == off[0] and on[4] == off[4] and off[0][0] is not None and off[0][0][1] is not None
    assert [c[:2] for c in off[1]] == [("risk_costs", 1)] and [c[:2] for c in on[1]] == [("risk_costs_batch", (1,))]
    for run in (off, on):       # its last level fell back on the planner's own engine
        assert [c[0] for c in run[2][0]] == ["risk_costs"] and run[2][1] == []


def test_closed_loop_is_identical(monkeypatch):
    """MultiAgentSimulation on the T-junction fixture, five steps, every planner with the "min_risk_cost" fallback: the plans are
    the same bytes with the flag on and off"""
    from tests.test_risk_planner import HARM, MASS, RISK
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)

    def run(flag):
        sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(), pipeline_groups=1,
                                              batched_risk_costs=flag)
        try:
            assert sim.batch.batched_risk_costs is flag
            kinds = {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}
            for a in sim.batch.agents:
                a.planner.set_risk_model(RISK, HARM, kinds, MASS)
                a.planner.set_risk_cost_weights(WEIGHTS, responsibility_mode="action_space")
                a.planner.set_fallback_selector("min_risk_cost")
            plans = []
            for _ in range(5):
                sim.step()
                plans.append(sim.plans.tobytes())
            return plans, [getattr(a.planner.optimal_trajectory, "uniqueId", None) for a in sim.batch.agents], sim.batch.launches
        finally:
            sim.close()

    assert run(True) == run(False)
