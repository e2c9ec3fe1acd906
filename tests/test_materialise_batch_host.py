"""The list pass on split lanes and over a whole agent batch (fx_set_materialise_lanes, fx_materialise_candidates_batch,
fx_last_materialise_info) without a GPU: the entry points are exported and declared, the ABI version stays, the
launcher constraint holds (one list launcher, no new one), they refuse what needs no device to refuse, and AgentBatchHip on the CPU
stand-in makes the per-agent calls it always made unless the flag is on AND the engine has materialise_batch."""
import ctypes as C
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, _lib, commonroad_xml as crx, multiagent
from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
from tests.oracle_engine import PackagingOracleEngine
from tests.test_launchers import stubbed_launchers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json")
NEW_SYMBOLS = {"fx_set_materialise_lanes": 2, "fx_materialise_candidates_batch": 5, "fx_last_materialise_info": 4}


def test_symbols_are_exported_and_declared():
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    for name, n_args in NEW_SYMBOLS.items():
        assert name in _lib.exported_symbols()
        f = getattr(L, name)
        assert f.restype is C.c_int32 and len(f.argtypes) == n_args, name
    assert re.search(r"int32_t\s+fx_set_materialise_lanes\s*\(\s*FxContext \*ctx, int32_t lanes\)", header)
    assert re.search(r"int32_t\s+fx_materialise_candidates_batch\s*\(\s*FxContext \*ctx, int32_t n_agents, const int32_t \*agents[^,]*,\s*"
                     r"const int64_t \*n_ids, const int64_t \*const \*ids\)", header)
    assert re.search(r"int32_t\s+fx_last_materialise_info\s*\(\s*FxContext \*ctx, int32_t \*lanes, int32_t \*launches, int32_t \*rows\)", header)
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays
    assert multiagent.BATCHED_MATERIALISE_DEFAULT is False
    assert PlannerConfig().sparse_lanes == 1


def test_one_list_launcher_and_no_new_one():
    """tests/context_owners.cpp and tests/batch_staging.cpp link every host source against the launcher stubs of fx_host_stubs.cpp
    and their own definitions: every launcher the host sources call is one of those, the list launcher under its one name"""
    stubs = stubbed_launchers()
    assert "fx_launch_eval_list" in stubs
    called = set()
    for src in os.listdir(CSRC):
        if src.startswith("fx_api") and src.endswith(".hip"):
            called |= set(re.findall(r"\b(fx_launch_\w+)\s*\(", open(os.path.join(CSRC, src)).read()))
    declared = set(re.findall(r"\b(fx_launch_\w+)\s*\(", open(os.path.join(CSRC, "fx_launch.h")).read()))
    assert "fx_launch_eval_list" in declared and len([n for n in declared if "eval_list" in n]) == 1
    # ... and it is the one launcher that takes the row table of the rows form
    decl = re.search(r"hipError_t fx_launch_eval_list\(([^;]*)\);", open(os.path.join(CSRC, "fx_launch.h")).read()).group(1)
    assert "const EvalListRow *d_rows, int n_rows, int lanes" in " ".join(decl.split())
    assert declared <= stubs and called <= stubs, (declared - stubs, called - stubs)
    used = set(re.findall(r"\b(fx_launch_\w+)\s*\(", open(os.path.join(CSRC, "fx_api_materialise.hip")).read()))
    assert used == {"fx_launch_eval_list"}
    for other in ("context_owners.cpp", "batch_staging.cpp"):
        text = open(os.path.join(ROOT, "tests", other)).read()
        defined = stubs | set(re.findall(r"hipError_t (fx_launch_\w+)\(", text))
        assert used <= defined, (other, used - defined)


def test_refusals_that_need_no_device():
    L = _lib.lib()
    fake = C.c_void_p(64)   # (never dereferenced: the arguments are looked at first)
    lst = np.array([1, 2], np.int64)
    n_ids = np.array([2, 0], np.int64)
    ids = np.array([lst.ctypes.data, 0], np.uint64)
    agents = np.array([0, 1], np.int32)
    guard = (lst.copy(), n_ids.copy(), ids.copy(), agents.copy())
    assert L.fx_materialise_candidates_batch(None, 2, agents.ctypes.data, n_ids.ctypes.data, ids.ctypes.data) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.fx_last_error()
    assert L.fx_materialise_candidates_batch(fake, -1, agents.ctypes.data, n_ids.ctypes.data, ids.ctypes.data) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"n_agents -1" in L.fx_last_error()
    assert L.fx_materialise_candidates_batch(fake, 2, agents.ctypes.data, None, ids.ctypes.data) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.fx_last_error()
    assert L.fx_materialise_candidates_batch(fake, 2, agents.ctypes.data, n_ids.ctypes.data, None) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.fx_last_error()
    assert L.fx_materialise_candidates_batch(fake, 0, agents.ctypes.data, n_ids.ctypes.data, ids.ctypes.data) == _abi.FX_OK
    assert L.fx_materialise_candidates_batch(fake, 0, None, None, None) == _abi.FX_OK   # nothing to do, nothing touched
    for lanes in (3, 2, 4, 16, 64, -1):
        assert L.fx_set_materialise_lanes(fake, lanes) == _abi.FX_ERR_INVALID_ARGUMENT
        assert str(lanes).encode() in L.fx_last_error()
    assert L.fx_set_materialise_lanes(None, 8) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_last_materialise_info(None, None, None, None) == _abi.FX_ERR_INVALID_ARGUMENT
    for a, b in zip(guard, (lst, n_ids, ids, agents)):
        assert np.array_equal(a, b)


class CountingEngine(PackagingOracleEngine):
    """the CPU stand-in with the per-agent materialise answered from the oracle's arrays (it computes every part whatever the
    step's mode is), and every call counted"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def materialise(self, ids, agent=0):
        self.calls.append(("materialise", agent, tuple(int(i) for i in ids)))
        out = self.last[agent][1]
        ids = np.asarray(ids, np.int64)
        return dict(planes=out["planes"][ids], lon=out["coeff_lon"][ids], lat=out["coeff_lat"][ids], tau_lat=out["tau_lat"][ids],
                    traj_len=out["traj_len"][ids], raw_costs=out["costmap"][ids], cost=out["cost"][ids], flags=out["flags"][ids],
                    boundary_step=None)


class BatchCountingEngine(CountingEngine):
    """the same with the batched method, answered by the per-agent one"""

    def materialise_batch(self, ids, agents=None):
        assert len(ids) == len(agents)
        self.calls.append(("batch", tuple(agents), tuple(tuple(int(i) for i in x) for x in ids)))
        res = [CountingEngine.materialise(self, x, a) for x, a in zip(ids, agents)]
        self.calls = [c for c in self.calls if c[0] != "materialise"]
        return res


def _run(factory, flag, steps=4):
    engines = []

    def make():
        engines.append(factory())
        return engines[-1]
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(sparse_bundle_k=8), number_of_agents=3,
                                          engine_factory=make, pipeline_groups=1, batched_materialise=flag)
    assert sim.batch.batched_materialise is bool(flag)
    agents = sim.batch.agents
    winners = []
    for _ in range(steps):
        sim.step()
        winners.append([a.optimal_trajectory.uniqueId if a.optimal_trajectory is not None else None for a in agents])
    calls = list(sim.batch.engine.calls)
    plans = sim.plans.tobytes()
    sim.close()
    return calls, winners, plans


def test_default_is_off():
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), engine_factory=CountingEngine)
    assert sim.batch.batched_materialise is multiagent.BATCHED_MATERIALISE_DEFAULT is False
    sim.close()


def test_engine_without_the_method_keeps_the_per_agent_calls():
    off = _run(CountingEngine, False)
    on = _run(CountingEngine, True)
    assert on == off
    assert [c[:2] for c in off[0]] == [("materialise", j) for j in range(4)] * 2     # four planners, two planning steps
    assert all(len(c[2]) >= 1 for c in off[0]) and all(w is not None for row in off[1] for w in row)


def test_batched_call_replaces_the_per_agent_calls():
    off = _run(CountingEngine, False)
    on = _run(BatchCountingEngine, True)
    assert on[1:] == off[1:]
    want = [("batch", (0, 1, 2, 3), tuple(tuple(sorted(set(c[2]))) for c in off[0][4 * s:4 * s + 4])) for s in range(2)]
    assert on[0] == want, on[0]
    assert _run(BatchCountingEngine, False)[0] == off[0]          # (off: the method is never called)
