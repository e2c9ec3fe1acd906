"""The collision-probability pass over a whole agent batch (fx_eval_prediction_prob_batch) without a GPU: the
entry point is exported and declared, refuses what needs no device to refuse, the ABI version stays, and AgentBatchHip on an engine
without `prediction_probability_batch` (the CPU stand-in) makes the per-agent calls it always made."""
import ctypes as C
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, _lib, commonroad_xml as crx, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
from tests.oracle_engine import PackagingOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")


def test_symbol_is_exported_and_declared():
    assert "fx_eval_prediction_prob_batch" in _lib.exported_symbols()
    L = _lib.lib()
    assert L.fx_eval_prediction_prob_batch.restype is C.c_int32 and len(L.fx_eval_prediction_prob_batch.argtypes) == 5
    header = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    assert re.search(r"int32_t\s+fx_eval_prediction_prob_batch\s*\(\s*FxContext \*ctx, int32_t n_agents, const int32_t \*agents", header)
    m = re.search(r"typedef struct FxPredProbBatchOutputs \{(.*?)\} FxPredProbBatchOutputs;", header, re.S)
    fields = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in _abi.FxPredProbBatchOutputs._fields_] == ["prob", "total", "best_index", "best_cost"]
    assert C.sizeof(_abi.FxPredProbBatchOutputs) == 4 * C.sizeof(C.c_void_p)
    L.fx_predprob_set_scratch_limit(0)      # (the test hook beside fx_predprob_set_chunk_steps)


def test_refusals_that_need_no_device():
    L = _lib.lib()
    params = (_abi.FxPredProbParams * 2)(_abi.FxPredProbParams(4.5, 1.6, 0), _abi.FxPredProbParams(4.5, 1.6, 0))
    prob, total = np.full(4, 7.0), np.full(4, 7.0)
    best_index, best_cost = np.full(2, 7, np.int64), np.full(2, 7.0)
    out = _abi.FxPredProbBatchOutputs(prob.ctypes.data, total.ctypes.data, best_index.ctypes.data, best_cost.ctypes.data)
    agents = np.array([0, 1], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    fake = C.c_void_p(64)   # (never dereferenced: params and out are looked at first)
    for ctx, p, o in ((None, params, C.byref(out)), (fake, None, C.byref(out)), (fake, params, None)):
        for n in (2, 0):
            assert L.fx_eval_prediction_prob_batch(ctx, n, agents, p, o) == _abi.FX_ERR_INVALID_ARGUMENT
            assert b"NULL" in L.fx_last_error()
    assert L.fx_eval_prediction_prob_batch(fake, -1, agents, params, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_eval_prediction_prob_batch(fake, 0, agents, params, C.byref(out)) == _abi.FX_OK      # nothing to do, nothing touched
    assert np.all(prob == 7.0) and np.all(total == 7.0) and np.all(best_index == 7) and np.all(best_cost == 7.0)
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays


class CountingEngine(PackagingOracleEngine):
    """the CPU stand-in with the per-agent pass answered from the oracle's own costs, and every call counted"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def set_risk_obstacles(self, tables, agent=0):
        self.calls.append(("tables", agent, int(tables["K"])))

    def prediction_probability(self, ego_length, ego_width, ids=None, agent=0, per_obstacle=False, source="probability"):
        self.calls.append(("pass", agent))
        out = self.last[agent][1]
        costed = (out["flags"] & _abi.FX_FLAG_COSTED) != 0
        return dict(prob=np.where(costed, 0.0, np.nan), total=np.where(costed, out["cost"], np.nan),
                    best_index=int(out["result"]["best_index"]), best_cost=float(out["result"].get("best_cost", np.nan)))


class BatchCountingEngine(CountingEngine):
    """the same with the batched method, answered by the per-agent one"""

    def prediction_probability_batch(self, ego_lengths, ego_widths, agents=None, source="probability"):
        self.calls.append(("batch", tuple(agents)))
        res = [CountingEngine.prediction_probability(self, ego_lengths[i], ego_widths[i], agent=a) for i, a in enumerate(agents)]
        self.calls = [c for c in self.calls if c[0] != "pass"]
        return res


def _run(factory, batched_passes, groups, steps=4):
    engines = []

    def make():
        engines.append(factory())
        return engines[-1]
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(prediction_cost="collision_probability"),
                                          engine_factory=make, pipeline_groups=groups, batched_passes=batched_passes)
    assert sim.batch.batched_passes is bool(batched_passes) and len(sim.batch.engines) == groups
    assert all(a.planner.batched_prediction_pass() for a in sim.batch.agents)
    winners = []
    for _ in range(steps):
        sim.step()
        winners.append([a.optimal_trajectory.uniqueId if a.optimal_trajectory is not None else -1 for a in sim.batch.agents])
    calls = [list(e.calls) for e in sim.batch.engines]
    plans, launches = sim.plans.tobytes(), sim.batch.launches   # (bytes: compared with ==)
    sim.close()
    return calls, winners, plans, launches


def test_default_follows_the_measurement():
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), engine_factory=CountingEngine)
    assert sim.batch.batched_passes is multiagent.BATCHED_PASSES_DEFAULT
    sim.close()


def test_engine_without_the_method_keeps_the_per_agent_calls():
    """batched_passes=True on an engine that lacks prediction_probability_batch: call for call what batched_passes=False makes"""
    for groups in (1, 2):
        off = _run(CountingEngine, False, groups)
        on = _run(CountingEngine, True, groups)
        assert on == off
        calls = [c for e in off[0] for c in e]
        n_agents = 5
        assert off[3] == 2 * groups                                           # two planning steps of four, one launch per group
        assert sum(c[0] == "pass" for c in calls) == 2 * n_agents and sum(c[0] == "tables" for c in calls) == 2 * n_agents
        for e in off[0]:                                                      # tables, then the pass, agent after agent
            assert all(a[0] == "tables" and b == ("pass", a[1]) for a, b in zip(e[0::2], e[1::2]))


def test_batched_call_replaces_the_per_agent_calls():
    """with the method: per engine group and planning step every agent's tables, then ONE batched call over exactly those agents;
    no per-agent pass; the same winners and plans"""
    for groups in (1, 2):
        off = _run(CountingEngine, False, groups)
        on = _run(BatchCountingEngine, True, groups)
        assert on[1:] == off[1:]
        for e in on[0]:
            n = len([c for c in e if c[0] == "tables"]) // 2
            want = ([("tables", j) for j in range(n)] + [("batch", tuple(range(n)))]) * 2
            assert [c[:2] for c in e] == want
        assert _run(BatchCountingEngine, False, groups)[0] == off[0]          # (off: the method is never called)
