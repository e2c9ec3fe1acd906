"""The plain risk pass over a whole agent batch (fx_eval_risk_batch) without a GPU: the entry point is
exported and declared, the struct's fields match _abi, it refuses what needs no device to refuse, the ABI version stays, and
AgentBatchHip on the CPU stand-in makes the per-agent calls it always made unless the flag is on AND the engine has risk_batch."""
import ctypes as C
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, _lib, commonroad_xml as crx, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
from tests.oracle_engine import PackagingOracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")
FIELDS = ["ego_risk", "obst_risk", "min_risk_index"]


def test_symbol_is_exported_and_declared():
    assert "fx_eval_risk_batch" in _lib.exported_symbols()
    L = _lib.lib()
    assert L.fx_eval_risk_batch.restype is C.c_int32 and len(L.fx_eval_risk_batch.argtypes) == 7
    header = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    assert re.search(r"int32_t\s+fx_eval_risk_batch\s*\(\s*FxContext \*ctx, int32_t n_agents, const int32_t \*agents", header)
    m = re.search(r"typedef struct FxRiskBatchOutputs \{(.*?)\} FxRiskBatchOutputs;", header, re.S)
    fields = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in _abi.FxRiskBatchOutputs._fields_] == FIELDS
    assert C.sizeof(_abi.FxRiskBatchOutputs) == 3 * C.sizeof(C.c_void_p)
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays
    assert multiagent.BATCHED_RISK_DEFAULT is False


def test_refusals_that_need_no_device():
    L = _lib.lib()
    pi64 = C.POINTER(C.c_int64)
    params = (_abi.FxRiskParams * 2)()
    arr = [np.full(4, 7.0), np.full(4, 7.0), np.full(2, 7, np.int64)]
    out = _abi.FxRiskBatchOutputs(*[a.ctypes.data for a in arr])
    agents = np.array([0, 1], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lst = np.array([1, 2], np.int64)
    n_ids = np.array([2, 0], np.int64).ctypes.data_as(pi64)
    ids = (pi64 * 2)(lst.ctypes.data_as(pi64), C.cast(None, pi64))
    fake = C.c_void_p(64)   # (never dereferenced: params and out are looked at first)
    for ctx, p, o in ((None, params, C.byref(out)), (fake, None, C.byref(out)), (fake, params, None)):
        for n in (2, 0):
            assert L.fx_eval_risk_batch(ctx, n, agents, p, n_ids, ids, o) == _abi.FX_ERR_INVALID_ARGUMENT
            assert b"NULL" in L.fx_last_error()
    for k in range(3):      # each output pointer
        bad = _abi.FxRiskBatchOutputs(*[None if j == k else a.ctypes.data for j, a in enumerate(arr)])
        assert L.fx_eval_risk_batch(fake, 2, agents, params, n_ids, ids, C.byref(bad)) == _abi.FX_ERR_INVALID_ARGUMENT
        assert b"output pointer is NULL" in L.fx_last_error()
    assert L.fx_eval_risk_batch(fake, -1, agents, params, n_ids, ids, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"n_agents -1" in L.fx_last_error()
    assert L.fx_eval_risk_batch(fake, 0, agents, params, n_ids, ids, C.byref(out)) == _abi.FX_OK   # nothing to do, nothing touched
    assert L.fx_eval_risk_batch(fake, 0, None, params, None, None, C.byref(out)) == _abi.FX_OK
    assert all(np.all(a == 7) for a in arr)


class CountingEngine(PackagingOracleEngine):
    """the CPU stand-in with the per-agent risk answered with zeros for the listed candidates, and every call counted"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def set_risk_obstacles(self, tables, agent=0):
        self.calls.append(("tables", agent, int(tables["K"])))

    def risk(self, params, ids=None, agent=0):
        self.calls.append(("risk", agent, None if ids is None else tuple(int(i) for i in ids)))
        n = len(self.last[agent][1]["flags"]) if ids is None else len(ids)
        return np.zeros(n), np.zeros(n), (int(np.min(ids)) if ids is not None and len(ids) else -1)


class BatchCountingEngine(CountingEngine):
    """the same with the batched method, answered by the per-agent one"""

    def risk_batch(self, params, ids=None, agents=None):
        assert len(params) == len(ids) == len(agents)
        self.calls.append(("batch", tuple(agents), tuple(None if x is None else tuple(int(i) for i in x) for x in ids)))
        res = [CountingEngine.risk(self, params[i], ids[i], a) for i, a in enumerate(agents)]
        self.calls = [c for c in self.calls if c[0] != "risk"]
        return res


def _run(factory, flag, groups, steps=4):
    from tests.test_risk_planner import HARM, MASS, RISK
    engines = []

    def make():
        engines.append(factory())
        return engines[-1]
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(log_risk=True), engine_factory=make,
                                          pipeline_groups=groups, batched_risk=flag)
    assert sim.batch.batched_risk is bool(flag) and len(sim.batch.engines) == groups
    agents = sim.batch.agents
    for a in agents:
        a.planner.set_risk_model(RISK, HARM, {i: "car" for i in list(sim.scenario.obstacles) + sim.agent_ids}, MASS)
    winners = []
    for _ in range(steps):
        sim.step()
        winners.append([(a.optimal_trajectory.uniqueId, a.optimal_trajectory._ego_risk, a.optimal_trajectory._obst_risk)
                        if a.optimal_trajectory is not None else None for a in agents])
    calls = [list(e.calls) for e in sim.batch.engines]
    plans, launches = sim.plans.tobytes(), sim.batch.launches   # (bytes: compared with ==)
    sim.close()
    return calls, winners, plans, launches


def test_default_is_off():
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), engine_factory=CountingEngine)
    assert sim.batch.batched_risk is multiagent.BATCHED_RISK_DEFAULT is False
    sim.close()


def test_engine_without_the_method_keeps_the_per_agent_calls():
    """batched_risk=True on an engine that lacks risk_batch: call for call what False makes"""
    for groups in (1, 2):
        off = _run(CountingEngine, False, groups)
        on = _run(CountingEngine, True, groups)
        assert on == off
        assert off[3] == 2 * groups                                           # two planning steps of four, one launch per group
        calls = [c for e in off[0] for c in e]
        # five planners, two planning steps: the tables, then the risk of the one winner, agent after agent
        assert sum(c[0] == "risk" for c in calls) == 2 * 5 and sum(c[0] == "tables" for c in calls) == 2 * 5
        for e in off[0]:
            assert all(a[0] == "tables" and b[:2] == ("risk", a[1]) and len(b[2]) == 1 for a, b in zip(e[0::2], e[1::2]))
        assert all(w is not None and w[1] == 0.0 and w[2] == 0.0 for row in off[1] for w in row)


def test_batched_call_replaces_the_per_agent_calls():
    """with the method: per engine group and planning step the tables of every planner that asks, then ONE batched call over exactly
    those agents with their one-id lists; no per-agent call; the same winners, risks and plans"""
    for groups in (1, 2):
        off = _run(CountingEngine, False, groups)
        on = _run(BatchCountingEngine, True, groups)
        assert on[1:] == off[1:]
        for e_on, e_off, n in zip(on[0], off[0], [5] if groups == 1 else [3, 2]):
            asked = [c[2] for c in e_off if c[0] == "risk"]                   # the winners of the per-agent path, in its order
            want = []
            for s in range(2):
                want += [("tables", j) for j in range(n)] + [("batch", tuple(range(n)), tuple(asked[s * n:(s + 1) * n]))]
            assert [c[:2] if c[0] == "tables" else c for c in e_on] == want, (groups, e_on)
        assert _run(BatchCountingEngine, False, groups)[0] == off[0]          # (off: the method is never called)
