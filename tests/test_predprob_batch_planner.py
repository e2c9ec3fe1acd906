"""AgentBatchHip(batched_passes=...) on the HIP engine: the closed loop of the T-junction's five planners with
prediction_cost="collision_probability" gives the same trajectories, costs, orders and cost-map entries whether the pass runs once
per engine group and step or once per agent; the calls are counted on the engines' methods.  The fifth planner also weights
`responsibility` and stays on its own pass; one planner is made to escalate and runs that level on its own engine."""
import os

import numpy as np
import pytest

from frenetix_motion_planner_amd import commonroad_xml as crx, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")
STEPS = 4          # two planning steps (every third step replans)
ESCALATES = 2      # the planner whose first level is thrown away in its first planning step


def _count(obj, name, log, tag):
    fn = getattr(obj, name)

    def counted(*a, **kw):
        log.append((tag, name, tuple(kw.get("agents") or ())))
        return fn(*a, **kw)
    setattr(obj, name, counted)


def _run(batched, groups):
    from tests.test_risk_planner import HARM, MASS, RISK
    cfg = PlannerConfig(prediction_cost="collision_probability", sampling_min=2, sampling_max=4)
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=cfg, pipeline_groups=groups, batched_passes=batched)
    log = []
    try:
        agents = sim.batch.agents
        assert len(agents) == 5 and len(sim.batch.engines) == groups
        fifth = agents[4].planner
        fifth.config.responsibility_mode = "action_space"
        fifth.set_risk_model(RISK, HARM, {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}, MASS)
        fifth.set_cost_function(dict(fifth.cost_weights, responsibility=0.5))
        assert [a.planner.batched_prediction_pass() for a in agents] == [True] * 4 + [False]
        for g, e in enumerate(sim.batch.engines):
            _count(e, "prediction_probability", log, ("group", g))
            _count(e, "prediction_probability_batch", log, ("group", g))
        p = agents[ESCALATES].planner
        _count(p.engine, "prediction_probability", log, ("own", ESCALATES))      # (the planner's own engine, created here)
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
                seen.append((k, None if best is None else (best.uniqueId, best.cost, best.costMap["prediction"], best.costMap.get("responsibility")),
                             step.cost.tobytes(), step.sorted_ids().tobytes(), step.engine is rp.engine))
        assert sim.batch.escalations == 1 and len(thrown) == 1
        return seen, sim.plans.tobytes(), log, sim.batch.launches
    finally:
        sim.close()


@pytest.mark.parametrize("groups", [1, 2])
def test_batched_passes_change_nothing_but_the_calls(groups):
    off = _run(False, groups)
    on = _run(True, groups)
    assert on[0] == off[0] and on[1] == off[1] and on[3] == off[3] == 2 * groups
    assert any(s[1] is not None and s[1][2][0] > 0 for s in on[0]), "no chosen trajectory with a positive collision probability"
    # off: every agent's pass from its own plan_consume -- 5 agents x 2 planning steps on the group engines -- and none batched
    group_calls = lambda log, name: [c for c in log if c[0][0] == "group" and c[1] == name]
    assert len(group_calls(off[2], "prediction_probability")) == 10 and not group_calls(off[2], "prediction_probability_batch")
    # on: one batched call per engine group and planning step over exactly the four planners that run the pass alone; the
    # per-agent method only for the fifth planner, from its responsibility pass
    batched = group_calls(on[2], "prediction_probability_batch")
    assert len(batched) == 2 * groups
    # (two groups: agents 0 - 2 and 3 - 4, the fifth planner the second group's local agent 1)
    for g in range(groups):
        mine = [c[2] for c in batched if c[0] == ("group", g)]
        want = tuple(j for j in range(3 if groups == 2 and g == 0 else (2 if groups == 2 else 5)) if not (g == groups - 1 and j == (4 if groups == 1 else 1)))
        assert mine == [want, want], (g, mine)
    assert len(group_calls(on[2], "prediction_probability")) == 2       # (the fifth planner's two steps)
    # the escalated level ran on the planner's own engine, with its own pass, in both runs
    own = lambda log: [c for c in log if c[0][0] == "own"]
    assert own(on[2]) == own(off[2]) == [(("own", ESCALATES), "prediction_probability", ())]
    assert [s[4] for s in on[0] if s[0] == ESCALATES][0] is True
