"""AgentBatchHip(batched_responsibility=...) on the HIP engine: the closed loop of the T-junction's five
planners gives the same trajectories, costs, orders, cost-map entries, risk fields and plans whether the responsibility pass runs
once per engine group and step or once per agent, with batched_passes on or off; the calls are counted on the engines' methods.
Planners 0 - 2 weight `responsibility` (0 and 1 in action-space mode, 2 in reach-set mode), planner 3 weights it AND runs
prediction_cost="collision_probability", planner 4 runs the collision probability alone; one planner is made to escalate and runs
that level on its own engine with its own per-agent pass."""
import os
import types

import numpy as np
import pytest

from frenetix_motion_planner_amd import commonroad_xml as crx, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")
STEPS = 4          # two planning steps (every third step replans)
ESCALATES = 1      # the planner whose first level is thrown away in its first planning step
NAMES = ("responsibility_cost", "responsibility_cost_batch", "prediction_probability", "prediction_probability_batch")


class _EveryStep(dict):
    """reach_sets[time_step]: the same sets at every time step"""

    def __missing__(self, key):
        return self["any"]


def _count(obj, name, log, tag):
    fn = getattr(obj, name)

    def counted(*a, **kw):
        log.append((tag, name, tuple(kw.get("agents") or ())))
        return fn(*a, **kw)
    setattr(obj, name, counted)


def _run(batched_passes, batched_responsibility, groups):
    from tests.test_risk_planner import HARM, MASS, RISK
    cfg = PlannerConfig(sampling_min=2, sampling_max=4)
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=cfg, pipeline_groups=groups, batched_passes=batched_passes,
                                          batched_responsibility=batched_responsibility)
    log = []
    try:
        agents = sim.batch.agents
        assert len(agents) == 5 and len(sim.batch.engines) == groups
        kinds = {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}
        for k, a in enumerate(agents):
            p = a.planner
            if k >= 3:
                p.config.prediction_cost = "collision_probability"
            if k == 4:
                continue
            p.config.responsibility_mode = "reach_set" if k == 2 else "action_space"
            p.set_risk_model(RISK, HARM, kinds, MASS)
            if k == 2:   # (as tests/test_responsibility_planner.py builds one: a part around everything at t = 0, a half plane later)
                other = next(i for i in sim.agent_ids if i in sim.scenario.obstacles and i != a.id)
                x, y = p.x_0.position
                big = np.array([[-1e4, -1e4], [1e4, -1e4], [1e4, 1e4], [-1e4, 1e4]])
                half = np.array([[x, y - 1e3], [x + 1e3, y - 1e3], [x + 1e3, y + 1e3], [x, y + 1e3]])
                p.set_reach_set(types.SimpleNamespace(reach_sets=_EveryStep(any={other: [{0.0: big}, {0.3: half}, {1.0: half[:3]}]})))
            p.set_cost_function(dict(p.cost_weights, responsibility=0.5))
        assert [a.planner.batched_responsibility_pass() for a in agents] == [True] * 4 + [False]
        assert [a.planner.batched_prediction_pass() for a in agents] == [False] * 4 + [True]
        for g, e in enumerate(sim.batch.engines):
            for name in NAMES:
                _count(e, name, log, ("group", g))
        p = agents[ESCALATES].planner
        for name in NAMES:
            _count(p.engine, name, log, ("own", ESCALATES))      # (the planner's own engine, created here)
        consume, thrown = p.plan_consume, []

        def first_level_finds_nothing(*a, **kw):
            best = consume(*a, **kw)
            if not thrown:
                thrown.append(best)
                return None
            return best
        p.plan_consume = first_level_finds_nothing
        seen = []
        for _ in range(STEPS):
            sim.step()
            for k, a in enumerate(agents):
                rp, step, best = a.planner, a.planner.last_step, a.planner.optimal_trajectory
                seen.append((k, None if best is None else (best.uniqueId, best.cost, best.costMap["prediction"], best.costMap.get("responsibility"),
                                                           best._ego_risk, best._obst_risk),
                             step.cost.tobytes(), step.sorted_ids().tobytes(), step.engine is rp.engine))
        assert sim.batch.escalations == 1 and len(thrown) == 1
        return seen, sim.plans.tobytes(), log, sim.batch.launches
    finally:
        sim.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_batched_responsibility_changes_nothing_but_the_calls(groups):
    off = _run(False, False, groups)
    both = _run(True, True, groups)
    resp = _run(False, True, groups)
    for on in (both, resp):
        assert on[0] == off[0] and on[1] == off[1] and on[3] == off[3] == 2 * groups
    entries = [s[1][3] for s in off[0] if s[1] is not None and s[0] < 4]
    assert entries and all(e is not None for e in entries)
    assert any(e[0] != 0 for e in entries), "no chosen trajectory with a responsibility cost"
    assert all(s[1][4] is not None for s in off[0] if s[1] is not None and s[0] < 4 and not s[4])   # (_ego_risk of the pass)
    calls = lambda run, name, where="group": [c for c in run[2] if c[0][0] == where and c[1] == name]
    # off: the calls of today -- four planners x two planning steps, each from its own plan_consume; the collision probability per
    # agent for planner 3 (inside its responsibility pass) and planner 4
    assert len(calls(off, "responsibility_cost")) == 8 and not calls(off, "responsibility_cost_batch")
    assert len(calls(off, "prediction_probability")) == 4 and not calls(off, "prediction_probability_batch")
    # on: one batched call per engine group and planning step over exactly the planners it serves, no per-agent pass on the group
    # engines; the collision probability of planner 3 as ONE further batched call over that subset
    # (two groups: agents 0 - 2 and 3 - 4, planners 3 and 4 the second group's local agents 0 and 1)
    served = [(0, 1, 2, 3)] if groups == 1 else [(0, 1, 2), (0,)]
    third = [(3,)] if groups == 1 else [(), (0,)]
    fourth = [(4,)] if groups == 1 else [(), (1,)]
    for on in (both, resp):
        assert not calls(on, "responsibility_cost")
        for g in range(groups):
            mine = [c[2] for c in calls(on, "responsibility_cost_batch") if c[0] == ("group", g)]
            assert mine == [served[g]] * 2, (g, mine)
    for g in range(groups):
        mine = [c[2] for c in calls(both, "prediction_probability_batch") if c[0] == ("group", g)]
        assert sorted(mine) == sorted(([third[g]] if third[g] else []) * 2 + ([fourth[g]] if fourth[g] else []) * 2), (g, mine)
        mine = [c[2] for c in calls(resp, "prediction_probability_batch") if c[0] == ("group", g)]
        assert mine == ([third[g]] if third[g] else []) * 2, (g, mine)
    assert not calls(both, "prediction_probability") and len(calls(resp, "prediction_probability")) == 2   # (planner 4's own, flag off)
    # the escalated level ran on the planner's own engine, with its own per-agent pass, in every run
    for run in (off, both, resp):
        assert calls(run, "responsibility_cost", "own") == [(("own", ESCALATES), "responsibility_cost", ())]
        assert not calls(run, "responsibility_cost_batch", "own")
        assert [s[4] for s in run[0] if s[0] == ESCALATES][0] is True
