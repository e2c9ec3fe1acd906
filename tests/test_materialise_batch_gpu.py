"""Listed candidates of a whole agent batch in one call (fx_materialise_candidates_batch), held to the per-agent
call on the same context and step: every agent's set bit for bit (int64 views, NaNs included) at 1, 8 and 32 lanes -- each agent
runs the kernel variant its per-agent call runs, one launch per variant present -- and the readers and passes that consume a set
answer on a batch-made one as on a per-agent one."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, engine as engine_module, synthetic
from tests.test_hip_parity import hip_hulls
from tests.test_materialise_gpu import FORMS, SMALL_KW, id_lists, select_only

pytestmark = pytest.mark.gpu

LANES = (1, 8, 32)
# six agents that differ in variant and shape: obstacles, none, windowed costs, road boundary, a sampling matrix, S = 51 beside 31
SIX = [SMALL_KW, FORMS["no_obstacles"], FORMS["windowed_costs"], FORMS["road_boundary"], FORMS["matrix"], FORMS["horizon5"]]
WINDOWED, NO_OBSTACLE = 2, 1
ROW_KEYS = ("planes", "lon", "lat", "tau_lat", "traj_len", "raw_costs", "cost", "flags", "boundary_step")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same_rows(got, want, what=""):
    for k in ROW_KEYS:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)


@pytest.fixture(scope="module")
def six():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=6 * 4096, max_steps=60, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64, max_agents=6)
    inps = [select_only(kw) for kw in SIX]
    e.results = e.plan_batch(inps)   # (kept for test_the_step_is_untouched_behind_a_batch_call)
    yield e, inps
    e.close()


def variants(inps, agents, lanes):
    """the kernel variants (lanes, obstacle stage, windowed terms) among the listed agents"""
    out = set()
    for a in agents:
        extra = a == WINDOWED
        obst = a != NO_OBSTACLE
        out.add((1 if extra else lanes, obst, extra))
    return out


@pytest.mark.parametrize("lanes", LANES)
def test_batch_equals_the_per_agent_call(six, lanes):
    eng, inps = six
    eng.set_materialise_lanes(lanes)
    try:
        lists = [id_lists(i.n_candidates) for i in inps]
        for form in range(5):
            ids = [lists[a][form] for a in range(6)]
            want = [eng.materialise(ids[a], agent=a) for a in range(6)]
            for a in range(6):
                eng.materialise([], agent=a)   # (the batch makes every set afresh)
            got = eng.materialise_batch(ids)
            info = eng.last_materialise_info
            assert info["rows"] == 6 and info["launches"] == len(variants(inps, range(6), lanes)) <= 4, info
            assert info["lanes"] == lanes
            for a in range(6):
                assert_same_rows(got[a], want[a], (form, a))
        # a list of agents out of order: the others keep their sets
        some = [5, 0, 3]
        ids = [lists[a][2] for a in some]
        want = [eng.materialise(x, agent=a) for x, a in zip(ids, some)]
        kept = eng._read_materialised(lists[1][4], 1)
        got = eng.materialise_batch(ids, agents=some)
        info = eng.last_materialise_info
        assert info["rows"] == 3 and info["launches"] == len(variants(inps, some, lanes))
        for j, a in enumerate(some):
            assert_same_rows(got[j], want[j], a)
        assert_same_rows(eng._read_materialised(lists[1][4], 1), kept, "agent 1 kept")
        # one agent with an empty list: its set is gone, the others are kept
        eng.materialise_batch([[]], agents=[3])
        assert eng.last_materialise_info == dict(lanes=0, launches=0, rows=0)
        with pytest.raises(ValueError, match="status -2"):
            eng._read_materialised(ids[2], 3)
        assert_same_rows(eng._read_materialised(ids[0], 5), want[0], "agent 5 kept")
        assert_same_rows(eng._read_materialised(lists[1][4], 1), kept, "agent 1 kept")
    finally:
        eng.set_materialise_lanes(1)


def test_the_step_is_untouched_behind_a_batch_call(six):
    eng, inps = six
    before = ([eng.costs(agent=a) for a in range(6)], eng.topk(32), eng.step_info())
    for lanes in (8, 1):   # (at one lane the rows kernel's one-lane forms run, which the per-agent call never launches)
        eng.set_materialise_lanes(lanes)
        try:
            eng.materialise_batch([id_lists(i.n_candidates)[2] for i in inps])
            eng.materialise_batch([np.arange(i.n_candidates) for i in inps])
            # rows in another order than the agents: a row index is no agent index
            eng.materialise_batch([np.arange(inps[a].n_candidates) for a in (5, 0, 3)], agents=[5, 0, 3])
        finally:
            eng.set_materialise_lanes(1)
        after = ([eng.costs(agent=a) for a in range(6)], eng.topk(32), eng.step_info())
        for x, y in zip(before[0], after[0]):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
        for x, y in zip(before[1], after[1]):
            assert np.array_equal(x, y)
        assert before[2] == after[2]
        # the published result blocks of all six agents: counters, histogram, winner -- what plan_batch returned
        assert list(eng.finish()) == list(eng.results)


def test_package_and_risk_answer_on_a_batch_made_set(six):
    from frenetix_motion_planner_amd import risk
    from tests.test_risk_gpu import BASE, EGO, HARM, _predictions
    eng, inps = six
    every = [np.arange(i.n_candidates) for i in inps]
    rows = eng.materialise(every[0], agent=0)
    flags = rows["flags"]
    planes = {n: rows["planes"][:, _abi.PLANE_NAMES.index(n), :].copy() for n in ("x", "y", "theta", "v")}
    preds, typ = _predictions(planes, flags, np.random.default_rng(7))
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ), agent=0)
    params = risk.risk_params(BASE, HARM, **EGO)
    ok = np.nonzero((flags & 0xB) == 0xB)[0]
    ids = np.random.default_rng(3).choice(ok, size=min(100, len(ok)), replace=False)

    def answers():
        pkg = eng.materialised_package(int(ids[0]), 0.125, agent=0)
        fields = [(list(v) if hasattr(v, "__len__") else v) for v in (getattr(pkg._pkg, f) for f, _ in _abi.FxPackage._fields_)]
        return fields, pkg.block.copy(), eng.risk(params, ids, agent=0)

    eng.set_materialise_lanes(32)
    try:
        eng.materialise(ids, agent=0)
        want = answers()
        eng.materialise([], agent=0)
        eng.materialise_batch([ids, every[1][:7]], agents=[0, 1])
        got = answers()
    finally:
        eng.set_materialise_lanes(1)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2][0], want[2][0]) and np.array_equal(got[2][1], want[2][1]) and got[2][2] == want[2][2]


def test_refusals_leave_every_previous_set_readable():
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    L = lib()
    inps = [select_only(kw) for kw in SIX[:3]]
    with FrenetEngine(max_candidates=3 * 4096, max_steps=60, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64, max_agents=4) as e:
        e.plan_batch(inps)
        first_ids = [np.array([7, 3, 450]), np.array([2, 1]), np.array([9])]
        first = e.materialise_batch(first_ids)
        held = e.device_bytes

        def call(agents, lists):
            ag = np.asarray(agents, np.int32)
            n_ids = np.asarray([len(x) for x in lists], np.int64)
            keep = [np.ascontiguousarray(x, np.int64) for x in lists]
            addr = np.asarray([x.ctypes.data for x in keep], np.uint64)
            return L.fx_materialise_candidates_batch(e._ctx, len(agents), ag.ctypes.data, n_ids.ctypes.data, addr.ctypes.data)

        def untouched():
            assert L.fx_last_error()
            assert e.device_bytes == held
            for a in range(3):
                again = e._read_materialised(first_ids[a], a)
                for k in ROW_KEYS:
                    if first[a][k] is not None:
                        assert np.array_equal(_bits(again[k]), _bits(first[a][k])), (a, k)

        big = [np.arange(400)] * 4
        assert call([0, 1, 0], big[:3]) == _abi.FX_ERR_INVALID_ARGUMENT and b"twice" in L.fx_last_error()
        untouched()
        assert call([0, 1, 2, 3], big) == _abi.FX_ERR_INVALID_ARGUMENT    # one agent more than the last upload holds
        untouched()
        assert call([0, 1], [np.arange(400), np.array([3, inps[1].n_candidates])]) == _abi.FX_ERR_INVALID_ARGUMENT   # an id equal to C
        untouched()
        assert call([0], [np.arange(400)]) == _abi.FX_OK    # (the same lists are accepted once nothing is wrong)
        e.materialise_batch(first_ids)
        held = e.device_bytes
        e.update_state(e._state_update_of(inps[0]))
        assert call([1, 2], big[:2]) == _abi.FX_ERR_NOT_READY and L.fx_last_error()
        assert e.device_bytes == held
        e.evaluate()
        e.finish()
        assert call([1, 2], [np.array([5]), np.array([6])]) == _abi.FX_OK


def test_device_bytes_unchanged_until_the_first_call():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inps = [select_only(kw) for kw in SIX[:2]]
    with FrenetEngine(max_candidates=2 * 4096, max_agents=2) as a, FrenetEngine(max_candidates=2 * 4096, max_agents=2) as b:
        a.plan_batch(inps)
        b.plan_batch(inps)
        b.set_materialise_lanes(8)
        assert a.device_bytes == b.device_bytes
        b.materialise_batch([[1, 2, 3], [4]])
        grown = b.device_bytes
        assert grown > a.device_bytes
        b.materialise_batch([[5], [6]])
        assert b.device_bytes == grown   # grow-only: shorter lists reuse the blocks


# ---- beyond one wave of agents ----
def test_sixty_five_agents():
    """A = 65 with test_many_agents_gpu.py's scenes (grids of 63, 64, 65 and 130 candidates cycling, agent 0 returns nothing), run
    select-only: the winner plus the top-k row of topk(32) for each agent, no list for agent 64, every candidate for agents 0 and 63"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from tests.test_many_agents_gpu import NO_WINNER, agent_kw
    A = 65
    inps = [synthetic.make_inputs(hull_builder=hip_hulls(), write_bundle=False, write_costmap=False, **agent_kw(a)) for a in range(A)]
    with FrenetEngine(max_candidates=A * 256, max_steps=31, max_ref_knots=1024, max_obstacles=8, max_pred_steps=64, max_agents=A) as e:
        res = e.plan_batch(inps)
        top = e.topk(32)[1]
        ids = []
        for a in range(A):
            keep = ([int(res[a]["best_index"])] if res[a]["best_index"] >= 0 else []) + [int(g) for g in top[a] if g >= 0]
            ids.append(np.asarray(keep, np.int64))
        ids[64] = np.zeros(0, np.int64)
        ids[0], ids[63] = np.arange(inps[0].n_candidates), np.arange(inps[63].n_candidates)
        n_rows = sum(len(x) > 0 for x in ids)
        assert n_rows == A - len(NO_WINNER)   # (agent 0 of them has its every candidate listed, agent 64 has no list; the others' lists are empty)
        for lanes in (1, 32):
            e.set_materialise_lanes(lanes)
            want = [e.materialise(ids[a], agent=a) for a in range(A)]
            for a in range(A):
                e.materialise([], agent=a)
            got = e.materialise_batch(ids)
            info = e.last_materialise_info
            assert info["rows"] == n_rows and 1 <= info["launches"] <= 4 and info["lanes"] == lanes, info
            for a in range(A):
                assert_same_rows(got[a], want[a], (lanes, a))
            with pytest.raises(ValueError, match="status -2"):
                e._read_materialised(np.array([0]), 64)


# ---- planner level ----
class CountingEngine(engine_module.FrenetEngine):
    """the HIP engine with its two materialise entrances counted"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def materialise(self, ids, agent=0):
        self.calls.append(("materialise", int(agent), len(ids)))
        return super().materialise(ids, agent)

    def materialise_batch(self, ids, agents=None):
        self.calls.append(("batch", tuple(agents), tuple(len(x) for x in ids)))
        return super().materialise_batch(ids, agents)


def _run_sim(monkeypatch, tmp, flag):
    import os
    from frenetix_motion_planner_amd import commonroad_xml as crx, logging_formats as lf, multiagent
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
    from tests.test_materialise_gpu import _pair_columns
    from tests.test_risk_batch_planner import FIXTURE, _rows

    monkeypatch.setattr(engine_module, "FrenetEngine", CountingEngine)
    sim = multiagent.MultiAgentSimulation(crx.read_scenario_json(FIXTURE), config=PlannerConfig(sparse_bundle_k=8), number_of_agents=3,
                                          pipeline_groups=1, batched_materialise=flag)
    sim.shared_packing = False     # (the loggers write the predictions out: plain dicts)
    try:
        agents = sim.batch.agents
        assert len(agents) == 4 and sim.batch.batched_materialise is flag and isinstance(sim.batch.engine, CountingEngine)
        for k, a in enumerate(agents):
            a.planner.logger = lf.DataLoggingCosts(os.path.join(str(tmp), f"{flag}_{k}"), save_all_traj=False,
                                                   cost_params=dict(a.planner.cost_weights))
        selected, chosen = [], []
        for _ in range(4):     # two planning steps (every third step replans)
            sim.step()
            selected.append(sim.plans.tobytes())
            chosen.append([None if a.planner.optimal_trajectory is None else
                           (a.planner.optimal_trajectory.uniqueId, a.planner.last_step.result["best_index"],
                            [c.tobytes() for c in _pair_columns(a.planner.trajectory_pair)]) for a in agents])
        for a in agents:
            getattr(a.planner.logger, "close", lambda: None)()
        rows = [_rows(os.path.join(str(tmp), f"{flag}_{k}", "logs.csv")) for k in range(4)]
        own = [c for a in agents if a.planner._engine is not None for c in getattr(a.planner._engine, "calls", [])]
        return selected, chosen, rows, list(sim.batch.engine.calls), own, sim.batch.launches
    finally:
        sim.close()


def test_agent_batch_materialises_its_keep_lists_in_one_call(monkeypatch, tmp_path):
    off = _run_sim(monkeypatch, tmp_path, False)
    on = _run_sim(monkeypatch, tmp_path, True)
    assert on[0] == off[0] and on[1] == off[1]                      # the selections and the trajectory pairs, bit for bit
    assert all(c is not None for row in off[1] for c in row)
    assert on[2] == off[2] and all(len(r) >= 2 for r in off[2])     # the rows of every planner's logs.csv
    assert on[5] == off[5] == 2 and not off[4] and not on[4]        # two planning steps, nobody escalated
    # off: one per-agent materialise from each planner's _consume_result per planning step; on: ONE materialise_batch over the
    # four planners with the same keep lists, and no per-agent call
    assert [c[:2] for c in off[3]] == [("materialise", j) for j in range(4)] * 2, off[3]
    assert on[3] == [("batch", (0, 1, 2, 3), tuple(c[2] for c in off[3][4 * s:4 * s + 4])) for s in range(2)], on[3]
