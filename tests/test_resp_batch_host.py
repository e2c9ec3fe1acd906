"""The responsibility pass over a whole agent batch (fx_eval_responsibility_cost_batch) without a GPU: the
entry point is exported and declared, refuses what needs no device to refuse, the ABI version stays, and AgentBatchHip on the CPU
stand-in makes the per-agent calls it always made unless the flag is on AND the engine has the batched method."""
import ctypes as C
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, _lib, commonroad_xml as crx, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
from tests.oracle_engine import PackagingOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")
FIELDS = ["resp", "total", "ego_risk", "obst_risk", "best_index", "best_cost"]
NO_PREDICTIONS = 1     # the planner that is never handed predictions


def test_symbol_is_exported_and_declared():
    assert "fx_eval_responsibility_cost_batch" in _lib.exported_symbols()
    L = _lib.lib()
    assert L.fx_eval_responsibility_cost_batch.restype is C.c_int32 and len(L.fx_eval_responsibility_cost_batch.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    assert re.search(r"int32_t\s+fx_eval_responsibility_cost_batch\s*\(\s*FxContext \*ctx, int32_t n_agents, const int32_t \*agents", header)
    m = re.search(r"typedef struct FxRespCostBatchOutputs \{(.*?)\} FxRespCostBatchOutputs;", header, re.S)
    fields = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in _abi.FxRespCostBatchOutputs._fields_] == FIELDS
    assert C.sizeof(_abi.FxRespCostBatchOutputs) == 6 * C.sizeof(C.c_void_p)
    L.fx_risk_batch_set_scratch_limit(0)      # (the test hook beside fx_predprob_set_scratch_limit)
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays


def test_refusals_that_need_no_device():
    L = _lib.lib()
    params = (_abi.FxRiskParams * 2)()
    resp = (_abi.FxRespCostParams * 2)(_abi.FxRespCostParams(0.5, 1, None, None), _abi.FxRespCostParams(0.5, 1, None, None))
    arr = [np.full(4, 7.0) for _ in range(4)] + [np.full(2, 7, np.int64), np.full(2, 7.0)]
    out = _abi.FxRespCostBatchOutputs(*[a.ctypes.data for a in arr])
    agents = np.array([0, 1], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(64)   # (never dereferenced: params, resp and out are looked at first)
    for ctx, p, r, o in ((None, params, resp, C.byref(out)), (fake, None, resp, C.byref(out)), (fake, params, None, C.byref(out)),
                         (fake, params, resp, None)):
        for n in (2, 0):
            assert L.fx_eval_responsibility_cost_batch(ctx, n, agents, p, r, o) == _abi.FX_ERR_INVALID_ARGUMENT
            assert b"NULL" in L.fx_last_error()
    assert L.fx_eval_responsibility_cost_batch(fake, -1, agents, params, resp, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_eval_responsibility_cost_batch(fake, 0, agents, params, resp, C.byref(out)) == _abi.FX_OK   # nothing to do, nothing touched
    assert all(np.all(a == 7) for a in arr)


class CountingEngine(PackagingOracleEngine):
    """the CPU stand-in with the per-agent pass answered from the oracle's own costs with resp = 0, and every call counted"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def set_risk_obstacles(self, tables, agent=0):
        self.calls.append(("tables", agent, int(tables["K"])))

    def responsibility_cost(self, params, cost_params, weight, ids=None, agent=0, prediction="step"):
        self.calls.append(("pass", agent))
        out = self.last[agent][1]
        costed = (out["flags"] & _abi.FX_FLAG_COSTED) != 0
        zero = np.where(costed, 0.0, np.nan)
        return dict(resp=zero, total=np.where(costed, out["cost"], np.nan), ego_risk=zero.copy(), obst_risk=zero.copy(),
                    best_index=int(out["result"]["best_index"]), best_cost=float(out["result"].get("best_cost", np.nan)), prediction=None)


class BatchCountingEngine(CountingEngine):
    """the same with the batched method, answered by the per-agent one"""

    def responsibility_cost_batch(self, params, cost_params, weights, agents=None, prediction="step"):
        assert len(params) == len(cost_params) == len(weights) == len(agents) == len(prediction)
        self.calls.append(("batch", tuple(agents)))
        res = [CountingEngine.responsibility_cost(self, params[i], cost_params[i], weights[i], agent=a) for i, a in enumerate(agents)]
        self.calls = [c for c in self.calls if c[0] != "pass"]
        return res


def _run(factory, flag, groups, steps=4, **cfg):
    from tests.test_risk_planner import HARM, MASS, RISK
    engines = []

    def make():
        engines.append(factory())
        return engines[-1]
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(responsibility_mode="action_space", **cfg),
                                          engine_factory=make, pipeline_groups=groups, batched_responsibility=flag)
    assert sim.batch.batched_responsibility is bool(flag) and len(sim.batch.engines) == groups
    agents = sim.batch.agents
    for a in agents:
        p = a.planner
        p.set_risk_model(RISK, HARM, {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}, MASS)
        p.set_cost_function(dict(p.cost_weights, responsibility=0.5))
        assert p.batched_responsibility_pass() and not p.batched_prediction_pass()
    lone = agents[NO_PREDICTIONS]
    lone.update_planner = lambda scenario, predictions, f=lone.update_planner: f(scenario, None)
    winners, entries = [], []
    for _ in range(steps):
        sim.step()
        winners.append([a.optimal_trajectory.uniqueId if a.optimal_trajectory is not None else -1 for a in agents])
        entries.append([a.optimal_trajectory.costMap.get("responsibility") if a.optimal_trajectory is not None else None for a in agents])
    calls = [list(e.calls) for e in sim.batch.engines]
    plans, launches = sim.plans.tobytes(), sim.batch.launches   # (bytes: compared with ==)
    sim.close()
    return calls, winners, plans, launches, entries


def test_default_follows_the_measurement():
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), engine_factory=CountingEngine)
    assert sim.batch.batched_responsibility is multiagent.BATCHED_RESPONSIBILITY_DEFAULT
    assert sim.batch.batched_passes is multiagent.BATCHED_PASSES_DEFAULT
    sim.close()


def test_engine_without_the_method_keeps_the_per_agent_calls():
    """batched_responsibility=True on an engine that lacks responsibility_cost_batch: call for call what False makes"""
    for groups in (1, 2):
        off = _run(CountingEngine, False, groups)
        on = _run(CountingEngine, True, groups)
        assert on == off
        calls = [c for e in off[0] for c in e]
        assert off[3] == 2 * groups                                           # two planning steps of four, one launch per group
        # four planners with predictions, two planning steps: tables, then the pass, agent after agent
        assert sum(c[0] == "pass" for c in calls) == 2 * 4 and sum(c[0] == "tables" for c in calls) == 2 * 4
        for e in off[0]:
            assert all(a[0] == "tables" and b == ("pass", a[1]) for a, b in zip(e[0::2], e[1::2]))
        # the planner without predictions: no pass, the term 0.0
        assert all(row[NO_PREDICTIONS] == (0.0, 0.0) for row in off[4])
        assert all(row[k] is not None and row[k][0] == 0.0 for row in off[4] for k in range(5))


def test_batched_call_replaces_the_per_agent_calls():
    """with the method: per engine group and planning step the tables of every planner whose preparation returns parameters, then ONE
    batched call over exactly those agents; no per-agent pass; the planner without predictions is left out; the same winners and plans"""
    for groups in (1, 2):
        off = _run(CountingEngine, False, groups)
        on = _run(BatchCountingEngine, True, groups)
        assert on[1:] == off[1:]
        assert all(row[NO_PREDICTIONS] == (0.0, 0.0) for row in on[4])
        first = 0
        for e, n in zip(on[0], [5] if groups == 1 else [3, 2]):   # (two groups: agents 0 - 2 and 3 - 4)
            served = tuple(j for j in range(n) if first + j != NO_PREDICTIONS)
            want = ([("tables", j) for j in served] + [("batch", served)]) * 2
            assert [c[:2] for c in e] == want, (groups, e)
            first += n
        assert _run(BatchCountingEngine, False, groups)[0] == off[0]          # (off: the method is never called)


def test_batched_prediction_pass_is_what_it_was():
    """the configurations of tests/test_predprob_batch_host.py and tests/test_predprob_batch_planner.py: the collision probability
    alone -- true; with `responsibility` weighted as well -- false"""
    from tests.test_risk_planner import HARM, MASS, RISK
    for cfg in (PlannerConfig(prediction_cost="collision_probability"),
                PlannerConfig(prediction_cost="collision_probability", sampling_min=2, sampling_max=4)):
        sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=cfg, engine_factory=CountingEngine)
        try:
            agents = sim.batch.agents
            assert all(a.planner.batched_prediction_pass() and not a.planner.batched_responsibility_pass() for a in agents)
            fifth = agents[4].planner
            fifth.config.responsibility_mode = "action_space"
            fifth.set_risk_model(RISK, HARM, {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}, MASS)
            fifth.set_cost_function(dict(fifth.cost_weights, responsibility=0.5))
            assert [a.planner.batched_prediction_pass() for a in agents] == [True] * 4 + [False]
            assert [a.planner.batched_responsibility_pass() for a in agents] == [False] * 4 + [True]
        finally:
            sim.close()
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), engine_factory=CountingEngine)
    assert not any(a.planner.batched_prediction_pass() or a.planner.batched_responsibility_pass() for a in sim.batch.agents)
    sim.close()
