"""AgentBatchHip(batched_risk=...) on the HIP engine: the planners' risk evaluations -- log_risk's one-id
list of the winner, the whole-candidate form of the "min_risk" fallback and of emergency_mode "min_risk" -- give the same
trajectories, risk bits and log rows whether they run as ONE risk_batch per engine group and planning step or as one risk call per
agent; the calls are counted on an engine subclass."""
import os

import numpy as np
import pytest

from frenetix_motion_planner_amd import commonroad_xml as crx, engine as engine_module, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")
STEPS = 7          # three planning steps (every third step replans)


class CountingEngine(engine_module.FrenetEngine):
    """the HIP engine with its two risk entrances counted"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def risk(self, params, ids=None, agent=0):
        self.calls.append(("risk", int(agent), None if ids is None else len(ids)))
        return super().risk(params, ids, agent)

    def risk_batch(self, params, ids=None, agents=None):
        self.calls.append(("risk_batch", tuple(agents), tuple(None if x is None else len(x) for x in ids)))
        return super().risk_batch(params, ids, agents)


def _rows(path):
    """the rows of a logs.csv without their second field, the planning time: a wall-clock figure"""
    return [";".join(f for k, f in enumerate(line.split(";")) if k != 1) for line in open(path).read().splitlines()[1:]]


def _run_fixture(monkeypatch, tmp, flag, groups):
    from frenetix_motion_planner_amd import logging_formats as lf
    from tests.test_risk_planner import HARM, MASS, RISK
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(log_risk=True), pipeline_groups=groups,
                                          batched_risk=flag)
    sim.shared_packing = False     # (the loggers write the predictions out: plain dicts)
    try:
        agents = sim.batch.agents
        assert len(agents) == 5 and len(sim.batch.engines) == groups and sim.batch.batched_risk is flag
        assert all(isinstance(e, CountingEngine) for e in sim.batch.engines)
        kinds = {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}
        for k, a in enumerate(agents):
            p = a.planner
            p.set_risk_model(RISK, HARM, kinds, MASS)
            p.logger = lf.DataLoggingCosts(os.path.join(str(tmp), f"{flag}_{groups}_{k}"), save_all_traj=False, cost_params=dict(p.cost_weights))
        selected, chosen = [], []
        for _ in range(STEPS):
            sim.step()
            selected.append(sim.plans.tobytes())     # (x, y, orientation, velocity of every agent's selected state list)
            chosen.append([None if a.planner.optimal_trajectory is None else
                           (a.planner.optimal_trajectory.uniqueId, np.float64(a.planner.optimal_trajectory._ego_risk).tobytes(),
                            np.float64(a.planner.optimal_trajectory._obst_risk).tobytes()) for a in agents])
        for a in agents:
            getattr(a.planner.logger, "close", lambda: None)()
        rows = [_rows(os.path.join(str(tmp), f"{flag}_{groups}_{k}", "logs.csv")) for k in range(5)]
        own = [c for a in agents if a.planner._engine is not None for c in getattr(a.planner._engine, "calls", [])]
        return selected, chosen, rows, [list(e.calls) for e in sim.batch.engines], sim.plans.tobytes(), sim.batch.launches, own
    finally:
        sim.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_log_risk_on_the_fixture(monkeypatch, tmp_path, groups):
    off = _run_fixture(monkeypatch, tmp_path, False, groups)
    on = _run_fixture(monkeypatch, tmp_path, True, groups)
    assert on[0] == off[0] and on[4] == off[4] and on[5] == off[5] == 3 * groups     # the selected state lists, the plans, the launches
    assert on[1] == off[1]                                                          # uniqueId and the risks' bits of every chosen sample
    risks = [c for row in off[1] for c in row if c is not None]
    assert len(risks) == 5 * STEPS and all(np.isfinite(np.frombuffer(c[1])[0]) and np.isfinite(np.frombuffer(c[2])[0]) for c in risks)
    assert any(np.frombuffer(c[1])[0] > 0 for c in risks), "no chosen trajectory with a risk"
    assert on[2] == off[2] and all(len(r) >= 3 for r in off[2])                     # the rows of every planner's logs.csv
    assert all(row.split(";")[-1] != "" for r in off[2] for row in r)
    # off: one risk call per agent and planning step, each with its one winner; on: ONE risk_batch per group and planning step
    sizes = [5] if groups == 1 else [3, 2]
    for g, n in enumerate(sizes):
        assert off[3][g] == [("risk", j, 1) for j in range(n)] * 3, off[3][g]                       # (every planner found a trajectory)
        assert on[3][g] == [("risk_batch", tuple(range(n)), (1,) * n)] * 3, on[3][g]               # exactly one per planning step, zero risk
    assert not off[6] and not on[6]                                                 # (no planner escalated: no engine of its own)


class _Agent:
    """what AgentBatchHip asks of an agent, around one planner that plans in every step"""

    def __init__(self, ident, planner):
        self.id, self.planner, self.pair = ident, planner, None

    def needs_plan(self):
        return True

    def update_planner(self, scenario, predictions):
        pass

    def begin_step(self):
        return self.planner.plan_begin()

    def finish_step(self, pair, current_timestep=None):
        self.pair = pair
        return (pair[0] if pair else None), 0

    def close(self):
        self.planner.close()


def _three(mode, escalating=None, **cfg):
    """two blocked planners (tests/test_planner_host.py: every feasible candidate collides) and a free one, single-level"""
    from tests.test_planner_host import blocked_planner
    from tests.test_risk_planner import HARM, MASS, RISK
    planners = []
    for k in range(3):
        # (the escalating one has a second level: its blocked first level goes on on the planner's own engine)
        rp = blocked_planner(engine=None, **dict(cfg, **(dict(sampling_min=2, sampling_max=4) if k == escalating else {})))
        wall = rp.predictions[5]
        wall["v_list"] = np.full(len(wall["pos_list"]), 0.5 + 0.25 * k)
        if k == 1:   # the free one: the wall stands far beside the road
            wall["pos_list"] = wall["pos_list"] + np.array([0.0, 60.0])
        rp.set_predictions({5: wall})
        rp.set_risk_model(RISK, HARM, {5: "car"}, MASS)
        if mode == "fallback":
            rp.set_fallback_selector("min_risk")
        planners.append(rp)
    return planners


def _run_three(mode, flag, escalating=None):
    cfg = dict(emergency_selection=True, emergency_mode="min_risk") if mode == "emergency" else {}
    planners = _three(mode, escalating, **cfg)
    cap = max(4096, max(p.max_candidates_per_step() for p in planners))
    batch = multiagent.AgentBatchHip([_Agent(10 + k, p) for k, p in enumerate(planners)], max_candidates=cap, pipeline_groups=1,
                                     batched_risk=flag)
    eng = batch.engine
    assert isinstance(eng, CountingEngine)
    try:
        batch.step(0, {})
        out = []
        for p in planners:
            best = p.optimal_trajectory
            out.append(None if best is None else (best.uniqueId, None if best._ego_risk is None else np.float64(best._ego_risk).tobytes(),
                                                  None if best._obst_risk is None else np.float64(best._obst_risk).tobytes()))
        own = [list(getattr(p._engine, "calls", [])) if p._engine is not None else [] for p in planners]
        steps = [p.last_step.result["best_index"] for p in planners]
        return out, list(eng.calls), own, batch.escalations, steps
    finally:
        batch.close()


@pytest.mark.parametrize("mode", ["fallback", "emergency"])
def test_min_risk_paths(mode, monkeypatch):
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)
    off = _run_three(mode, False)
    on = _run_three(mode, True)
    assert on[0] == off[0] and on[4] == off[4]
    assert off[4][0] == -1 and off[4][2] == -1 and off[4][1] >= 0       # two blocked, one free
    # the blocked ones chose by risk, and carry it; the free one chose by cost and carries none (no log_risk)
    assert all(off[0][k] is not None and off[0][k][1] is not None for k in (0, 2)) and off[0][1] is not None and off[0][1][1] is None
    # off: the whole-candidate evaluation as one per-agent call of each blocked planner over its feasible candidates
    assert [c[:2] for c in off[1]] == [("risk", 0), ("risk", 2)] and all(c[2] > 0 for c in off[1])
    # on: only the agents that need it, in the ONE call, without lists
    assert on[1] == [("risk_batch", (0, 2), (None, None))], on[1]
    assert off[3] == on[3] == 0


def test_an_escalating_planner_keeps_the_per_agent_path(monkeypatch):
    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)
    off = _run_three("fallback", False, escalating=0)
    on = _run_three("fallback", True, escalating=0)
    assert on[0] == off[0] and off[3] == on[3] == 1
    assert off[0][0] is not None and off[0][0][1] is not None          # its last level fell back to the lowest risk, on its own engine
    assert on[1] == [("risk_batch", (2,), (None,))] and [c[:2] for c in off[1]] == [("risk", 2)]
    for run in (off, on):
        assert [c[0] for c in run[2][0]] == ["risk"] and run[2][1] == [] and run[2][2] == []
