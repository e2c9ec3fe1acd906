"""Risk detail and risk costs of a whole agent batch (fx_eval_risk_costs_batch) without a GPU: the entry
point is exported and declared, the struct's fields match _abi, it refuses what needs no device to refuse, the ABI version stays,
the host-only build has the launcher's stub, and AgentBatchHip on the CPU stand-in makes the per-agent risk_costs calls it always
made unless the flag is on AND the engine has risk_costs_batch."""
import ctypes as C
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, _lib, multiagent
from tests.oracle_engine import PackagingOracleEngine
from tests.test_launchers import stubbed_launchers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["ego_risk", "obst_risk", "obst_harm_occ", "ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max", "bayes",
          "equality", "maximin", "ego", "responsibility", "total", "boundary_harm", "min_risk_index", "min_cost_index"]


def test_symbol_is_exported_and_declared():
    assert "fx_eval_risk_costs_batch" in _lib.exported_symbols()
    L = _lib.lib()
    assert L.fx_eval_risk_costs_batch.restype is C.c_int32 and len(L.fx_eval_risk_costs_batch.argtypes) == 8
    header = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    assert re.search(r"int32_t\s+fx_eval_risk_costs_batch\s*\(\s*FxContext \*ctx, int32_t n_agents, const int32_t \*agents", header)
    assert re.search(r"const FxRiskCostParams \*const \*cost", header)
    m = re.search(r"typedef struct FxRiskCostBatchOutputs \{(.*?)\} FxRiskCostBatchOutputs;", header, re.S)
    fields = re.findall(r"\*(\w+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [n for n, _ in _abi.FxRiskCostBatchOutputs._fields_] == FIELDS
    assert fields == [n for n, _ in _abi.FxRiskOutputs._fields_]              # the per-agent structure's fields, in its order
    assert C.sizeof(_abi.FxRiskCostBatchOutputs) == 16 * C.sizeof(C.c_void_p)
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays
    assert multiagent.BATCHED_RISK_COSTS_DEFAULT is False
    # the launcher has a stub in the host-only build, like its siblings (and is declared once, nowhere weak: tests/test_launchers.py)
    assert "fx_launch_risk_costs_batch" in stubbed_launchers()
    assert L.fx_last_risk_costs_batch_rounds(None) == -1


def test_refusals_that_need_no_device():
    L = _lib.lib()
    pi64, pcp = C.POINTER(C.c_int64), C.POINTER(_abi.FxRiskCostParams)
    params = (_abi.FxRiskParams * 2)()
    arr = [np.full(4, 7.0) for _ in range(14)] + [np.full(2, 7, np.int64), np.full(2, 7, np.int64)]
    out = _abi.FxRiskCostBatchOutputs(*[a.ctypes.data for a in arr])
    agents = np.array([0, 1], np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    lst = np.array([1, 2], np.int64)
    n_ids = np.array([2, 0], np.int64).ctypes.data_as(pi64)
    ids = (pi64 * 2)(lst.ctypes.data_as(pi64), C.cast(None, pi64))
    cp = _abi.FxRiskCostParams()
    cost = (pcp * 2)(C.pointer(cp), C.cast(None, pcp))
    fake = C.c_void_p(64)   # (never dereferenced: params and out are looked at first)
    call = L.fx_eval_risk_costs_batch
    for ctx, p, o in ((None, params, C.byref(out)), (fake, None, C.byref(out)), (fake, params, None)):
        for n in (2, 0):
            assert call(ctx, n, agents, p, cost, n_ids, ids, o) == _abi.FX_ERR_INVALID_ARGUMENT
            assert b"NULL" in L.fx_last_error()
    assert call(fake, -1, agents, params, cost, n_ids, ids, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"n_agents -1" in L.fx_last_error()
    assert call(fake, 0, agents, params, cost, n_ids, ids, C.byref(out)) == _abi.FX_OK   # nothing to do, nothing touched
    assert call(fake, 0, None, params, None, None, None, C.byref(out)) == _abi.FX_OK
    assert all(np.all(a == 7) for a in arr)


class CountingEngine(PackagingOracleEngine):
    """the CPU stand-in with the per-agent risk_costs answered from the listed candidates alone, and every call counted"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def set_risk_obstacles(self, tables, agent=0):
        self.calls.append(("tables", agent, int(tables["K"])))

    def set_reach_sets(self, tables, agent=0):
        self.calls.append(("reach", agent))

    def risk_costs(self, params, cost_params, ids=None, agent=0):
        assert ids is not None and cost_params is not None
        ids = np.asarray(ids, np.int64)
        self.calls.append(("risk_costs", agent, tuple(int(i) for i in ids), int(cost_params.responsibility_mode)))
        pick = ids[(7 * (agent + 1)) % len(ids)]
        return dict(ego_risk=ids * 1e-3 + agent, obst_risk=ids * 2e-3 + agent, min_cost_index=int(pick), min_risk_index=int(ids[0]))


class BatchCountingEngine(CountingEngine):
    """the same with the batched method, the loop of the per-agent one"""

    def risk_costs_batch(self, params, cost_params, ids=None, agents=None):
        assert len(params) == len(cost_params) == len(ids) == len(agents)
        res = [CountingEngine.risk_costs(self, params[i], cost_params[i], ids[i], a) for i, a in enumerate(agents)]
        asked = [c for c in self.calls if c[0] == "risk_costs"][-len(agents):]
        self.calls = [c for c in self.calls if c[0] != "risk_costs"] + [("batch", tuple(agents), tuple(c[2] for c in asked), tuple(c[3] for c in asked))]
        return res


def _run(factory, flag, mode, steps=2, both=False):
    """three single-level planners on one engine, the first and the last blocked (every feasible candidate collides) with the
    "min_risk_cost" fallback, stepped `steps` times: (calls, chosen samples with their risks, the launches)"""
    from tests.test_planner_host import blocked_planner
    from tests.test_risk_batch_planner import _Agent
    from tests.test_risk_planner import HARM, MASS, RISK
    planners = []
    for k in range(3):
        rp = blocked_planner()
        wall = rp.predictions[5]
        wall["v_list"] = np.full(len(wall["pos_list"]), 0.5 + 0.25 * k)
        if k == 1:   # the free one: the wall stands far beside the road
            wall["pos_list"] = wall["pos_list"] + np.array([0.0, 60.0])
        rp.set_predictions({5: wall})
        rp.set_risk_model(RISK, HARM, {5: "car"}, MASS)
        rp.set_risk_cost_weights([1.0, 0.5, 2.0, 0.25, 1.5], mode)
        rp.set_fallback_selector("min_risk_cost")
        planners.append(rp)
    eng = factory()
    cap = max(4096, max(p.max_candidates_per_step() for p in planners))
    batch = multiagent.AgentBatchHip([_Agent(10 + k, p) for k, p in enumerate(planners)], max_candidates=cap, engine=eng,
                                     batched_risk_costs=flag, **(dict(batched_risk=True) if both else {}))
    assert batch.batched_risk_costs is bool(flag) and batch.batched_risk is both
    chosen = []
    for t in range(steps):
        batch.step(t, {})
        chosen.append([None if p.optimal_trajectory is None else
                       (p.optimal_trajectory.uniqueId, p.optimal_trajectory._ego_risk, p.optimal_trajectory._obst_risk) for p in planners])
    calls, launches = list(eng.calls), batch.launches
    assert all(p._engine is None or not getattr(p._engine, "calls", []) for p in planners)
    return calls, chosen, launches


def test_default_is_off():
    batch = multiagent.AgentBatchHip([], max_candidates=64, engine=CountingEngine())
    assert batch.batched_risk_costs is multiagent.BATCHED_RISK_COSTS_DEFAULT is False
    assert "batched_risk_costs" in multiagent.MultiAgentSimulation.__init__.__code__.co_varnames


def test_engine_without_the_method_keeps_the_per_agent_calls():
    """batched_risk_costs=True on an engine that lacks risk_costs_batch: call for call what False makes"""
    for mode in ("action_space", None):
        off = _run(CountingEngine, False, mode)
        on = _run(CountingEngine, True, mode)
        assert on == off and off[2] == 2
        # two blocked planners, two steps: the tables, then the risk costs over every feasible candidate, agent after agent
        assert [c[:2] for c in off[0]] == [("tables", 0), ("risk_costs", 0), ("tables", 2), ("risk_costs", 2)] * 2
        assert all(len(c[2]) > 1 and c[3] == (1 if mode else 0) for c in off[0] if c[0] == "risk_costs")
        for row in off[1]:
            assert row[1] is not None and row[1][1] is None                   # the free one chose by cost and carries no risk
            for k in (0, 2):
                g = row[k][0]
                assert row[k][1] == g * 1e-3 + k and row[k][2] == g * 2e-3 + k   # the rows of the chosen candidate


def test_batched_call_replaces_the_per_agent_calls():
    """with the method: per step the tables of every planner that asks, then ONE batched call over exactly those agents with their
    lists; no per-agent call; the same selections with the same risks"""
    for mode in ("action_space", None):
        off = _run(CountingEngine, False, mode)
        on = _run(BatchCountingEngine, True, mode)
        assert on[1:] == off[1:]
        asked = [c for c in off[0] if c[0] == "risk_costs"]
        want = []
        for s in range(2):
            a, b = asked[2 * s], asked[2 * s + 1]
            want += [("tables", 0), ("tables", 2), ("batch", (0, 2), (a[2], b[2]), (a[3], b[3]))]
        assert [c[:2] if c[0] == "tables" else c for c in on[0]] == want, on[0]
        assert _run(BatchCountingEngine, False, mode)[0] == off[0]            # (off: the method is never called)
        # beside batched_risk on an engine without risk_batch: the same one call
        assert _run(BatchCountingEngine, True, mode, both=True) == on
