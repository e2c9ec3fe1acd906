"""TrajectorySample objects a caller keeps outlive their plan step: what they have not fetched yet is rescued -- one batched
engine read -- before the next evaluation overwrites the device buffers (PlanStepResult.rescue, StepRegistry; DESIGN.md
section 12).  The CPU tests drive the product's host layers on the oracle-backed stand-in engines (tests/oracle_engine.py);
the `gpu` ones repeat them on the real engine, where a kept sample must read, bit for bit, what a twin read BEFORE the next
step, and the oracle's first step at the project's tolerances (planes 1e-9 of the plane's scale, cost 1e-9 relative,
coefficients 1e-10)."""
import gc

import numpy as np
import pytest

from frenetix_motion_planner_amd import VehicleParams, _abi, synthetic
from frenetix_motion_planner_amd.trajectories import StepRegistry
from tests.handler_fixture import evaluate, make_handler
from tests.oracle_engine import OracleEngine, PackagingOracleEngine

STALE = "device data has been overwritten"
CART = ("x", "y", "theta", "v", "a", "kappa", "kappa_dot")                      # planes 0 .. 6
CURV = (("s", 7), ("d", 8), ("theta", 9), ("s_dot", 10), ("s_ddot", 11), ("d_dot", 12), ("d_ddot", 13))


# ------------------------------------------------------------------------------------------------ the frenetix route
def oracle_of(h):
    """the oracle's arrays of the handler's current step (obstacle hulls by the oracle's own builder)"""
    from oracle import oracle
    import copy
    inp = copy.copy(h._step.inputs)
    inp.obstacles = synthetic.pack_predictions(h._predictions(), 31, oracle.build_obstacle_hulls)
    return oracle.plan_step(inp, want_planes=True)


def picks(trajs, out, seed=11, n=5):
    """positions in the sorted list: the winner and n seeded picks among the candidates the oracle decides with margin >= 1e-9"""
    robust = [j for j, t in enumerate(trajs) if out["margin"][t.uniqueId] >= 1e-9]
    win = next(j for j in robust if trajs[j].uniqueId == out["result"]["best_index"])
    rest = [j for j in robust if j != win]
    return [win] + sorted(np.random.default_rng(seed).choice(rest, n, replace=False).tolist())


def read_all(t) -> dict:
    """every attribute the issue lists, as arrays / scalars"""
    c, cl = t.cartesian, t.curvilinear
    r = {"cart." + n: np.array(getattr(c, n)) for n in CART}
    r.update({"curv." + n: np.array(getattr(cl, n)) for n, _ in CURV})
    r["costMap"] = np.array([t.costMap[n] for n in t._step.inputs.cost_names])
    r["feasabilityMap"] = np.array([t.feasabilityMap[k] for k in sorted(t.feasabilityMap)])
    r["sampling_parameters"] = np.array(t.sampling_parameters)
    r["lon"], r["lat"] = np.array(t.trajectory_long.coeffs), np.array(t.trajectory_lat.coeffs)
    r["delta_tau"] = np.array([t.trajectory_lat.delta_tau])
    r["traj_len"] = np.array([t.actual_traj_length])
    r["cost"] = np.array([t.cost])
    return r


def expected(out, inp, m, g) -> dict:
    """the same from a step's oracle-shaped arrays"""
    r = {"cart." + n: out["planes"][g][k] for k, n in enumerate(CART)}
    r.update({"curv." + n: out["planes"][g][k] for n, k in CURV})
    w = inp.cost_weights
    r["costMap"] = np.array([(float(out["costmap"][g][k]), float(w[n] * out["costmap"][g][k])) for k, n in enumerate(inp.cost_names)])
    reasons = (int(out["flags"][g]) >> _abi.FX_REASON_SHIFT) & 0x7FF
    bits = {"Curvature Constraint": 5, "Yaw rate Constraint": 6, "Curvature Rate Constraint": 7, "Acceleration Constraint": 8}
    r["feasabilityMap"] = np.array([float((reasons >> bits[k]) & 1) for k in sorted(bits)])
    r["sampling_parameters"] = m[g]
    r["lon"], r["lat"] = out["coeff_lon"][g], out["coeff_lat"][g]
    r["delta_tau"] = np.array([out["tau_lat"][g]])
    r["traj_len"] = np.array([out["traj_len"][g]])
    r["cost"] = np.array([out["cost"][g]])
    return r


def same_bits(a: dict, b: dict):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k], np.float64), np.ascontiguousarray(b[k], np.float64)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), k


def within_tolerance(got: dict, ref: dict):
    """GPU against the oracle: planes 1e-9 of the plane's scale, cost 1e-9 relative, coefficients 1e-10; integers exact"""
    for k, b in ref.items():
        a, b = np.asarray(got[k], np.float64), np.asarray(b, np.float64)
        if k.startswith(("cart.", "curv.")):
            assert np.abs(a - b).max() <= 1e-9 * (1.0 + np.abs(b).max()), k
        elif k in ("cost", "costMap"):
            assert (np.abs(a - b) <= 1e-9 * np.maximum(np.abs(b), 1e-12)).all(), k
        elif k in ("lon", "lat", "delta_tau"):
            assert np.abs(a - b).max() <= 1e-10 * (1.0 + np.abs(b).max()), k
        else:
            assert np.array_equal(a, b), k


def frenetix_route(engine_factory, against_oracle_exactly):
    h, matrix = make_handler(engine_factory())
    twin, _ = make_handler(engine_factory())
    try:
        m1, m2 = matrix(), matrix(1.0, 10.5)
        for hh in (h, twin):
            hh.reset_Trajectories()
            evaluate(hh, m1)
        out1 = oracle_of(h)
        inp1 = h._step.inputs
        trajs = h.get_sorted_trajectories()
        assert len(trajs) == 800
        at = picks(trajs, out1)
        assert trajs[at[0]].uniqueId == out1["result"]["best_index"]
        kept = [trajs[j] for j in at]
        before = [read_all(twin.get_sorted_trajectories()[j]) for j in at]   # the twin reads while its step is fresh
        del trajs
        h.reset_Trajectories()
        evaluate(h, m2)
        assert h._step.inputs is not inp1
        for t, b in zip(kept, before):
            got = read_all(t)
            same_bits(got, b)
            ref = expected(out1, inp1, m1, t.uniqueId)
            if against_oracle_exactly:
                same_bits(got, ref)
            else:
                within_tolerance(got, ref)
        # the new step is a different one: the same candidate reads other values there
        g = kept[0].uniqueId
        assert not np.array_equal(h._step.sample(g).cartesian.x, kept[0].cartesian.x)
        # a candidate nobody held: the old error, as ever
        old = kept[0]._step
        free = next(i for i in range(800) if i not in {t.uniqueId for t in kept})
        with pytest.raises(RuntimeError, match=STALE):
            old.sample(free).cartesian
    finally:
        h.engine.close()
        twin.engine.close()


def test_frenetix_route_kept_samples_read_the_first_step():
    frenetix_route(OracleEngine, against_oracle_exactly=True)


@pytest.mark.gpu
def test_frenetix_route_kept_samples_read_the_first_step_gpu():
    frenetix_route(lambda: None, against_oracle_exactly=False)


def _counted(name):
    def f(self, *a, **k):
        self.reads += 1
        return getattr(OracleEngine, name)(self, *a, **k)
    return f


class CountingEngine(OracleEngine):
    """counts the calls of the read-back surface"""

    def __init__(self):
        super().__init__()
        self.reads = 0

    costs, boundary_steps, costmap = _counted("costs"), _counted("boundary_steps"), _counted("costmap")
    coeffs, sample, plane = _counted("coeffs"), _counted("sample"), _counted("plane")


class CandidatesOracle(CountingEngine):
    """... with the batched read-back of FrenetEngine (candidates) from the oracle's arrays, counted apart"""

    def __init__(self):
        super().__init__()
        self.batched = []

    def candidates(self, ids, agent=0):
        inp, out = self.last[agent]
        ids = np.asarray(ids, np.int64)
        self.batched.append(ids.tolist())
        co = np.concatenate([out["coeff_lon"][ids], out["coeff_lat"][ids], out["tau_lat"][ids][:, None]], axis=1)   # the coeffs13 block
        return dict(planes=out["planes"][ids].copy(), lon=co[:, :6], lat=co[:, 6:12], tau_lat=co[:, 12], traj_len=out["traj_len"][ids].astype(np.int32),
                    raw_costs=out["costmap"][ids].copy(), cost=out["cost"][ids].copy(), flags=out["flags"][ids].copy(), boundary_step=None)


def test_rescue_is_one_batched_read():
    """an engine with candidates(): ONE call for all held samples, nothing per sample; rows found by index"""
    h, matrix = make_handler(CandidatesOracle())
    m1 = matrix()
    h.reset_Trajectories()
    evaluate(h, m1)
    out1, inp1 = h.engine.last[0][1], h._step.inputs
    trajs = h.get_sorted_trajectories()
    kept = [trajs[j] for j in (700, 3, 41, 250)]        # (not in index order)
    del trajs
    gc.collect()
    reads = h.engine.reads
    h.reset_Trajectories()
    evaluate(h, matrix(1.0, 10.5))
    assert h.engine.batched == [sorted(t.uniqueId for t in kept)] and h.engine.reads == reads
    for t in kept:
        same_bits(read_all(t), expected(out1, inp1, m1, t.uniqueId))
    assert h.engine.batched == [sorted(t.uniqueId for t in kept)] and h.engine.reads == reads
    # rescue() on a fresh step, more samples taken afterwards: the reset reads those too
    step = h._step
    first = h.get_sorted_trajectories()[5]
    step.rescue()
    second = step.sample(first.uniqueId + 1 if first.uniqueId < 799 else 0)
    h.reset_Trajectories()
    assert sorted(step._snap_ids.tolist()) == sorted((first.uniqueId, second.uniqueId))
    assert second.cartesian.x.shape == (31,) and first.costMap


def test_only_what_is_held_is_rescued():
    h, matrix = make_handler(CountingEngine())
    h.reset_Trajectories()
    evaluate(h, matrix())
    trajs = h.get_sorted_trajectories()
    step = h._step
    keep = [trajs[3], trajs[500]]
    del trajs
    gc.collect()
    assert len(step.live_samples()) == 2
    h.reset_Trajectories()
    assert sorted(step._snap_ids.tolist()) == sorted(t.uniqueId for t in keep)
    assert len(step._snap["planes"]) == len(step._snap["cost"]) == 2
    assert keep[0].cartesian.x.shape == (31,) and keep[1].costMap
    # rescue() again and on a stale step: nothing happens
    snap = step._snap
    step.rescue()
    step.invalidate(rescue=True)
    assert step._snap is snap
    # nothing held: not one read-back call
    evaluate(h, matrix(1.0, 10.5))
    trajs = h.get_sorted_trajectories()
    step2 = h._step
    del trajs
    gc.collect()
    n = h.engine.reads
    h.reset_Trajectories()
    assert h.engine.reads == n and step2._snap is None and step2._stale


def test_retain_samples_off_restores_the_error():
    h, matrix = make_handler(CountingEngine())
    h.retain_samples = False
    h.reset_Trajectories()
    evaluate(h, matrix())
    kept = h.get_sorted_trajectories()[:3]
    n = h.engine.reads
    h.reset_Trajectories()
    evaluate(h, matrix(1.0, 10.5))
    assert h.engine.reads == n
    for attr in ("cartesian", "costMap", "trajectory_long"):
        with pytest.raises(RuntimeError, match=STALE):
            getattr(kept[0], attr)
    assert kept[0].feasabilityMap and kept[0].sampling_parameters.shape == (13,)   # (these never needed the device)


# ------------------------------------------------------------------------------------------------ the planner
def make_planner(engine, v0=10.0, **cfg):
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig, ReactivePlannerHip, ReactivePlannerState
    rp = ReactivePlannerHip(PlannerConfig(**cfg), VehicleParams(), engine=engine)
    ref = synthetic.reference_polyline("arc", 400, 0.5, 0.01)
    cs = synthetic.CoordinateSystem(ref)
    s0 = float(cs.ref_pos[40] + 0.1)
    x0 = ReactivePlannerState(time_step=0, position=cs.convert_to_cartesian_coords(s0, 0.2), orientation=float(cs.ref_theta[40]), velocity=v0)
    preds = synthetic.synthetic_predictions(cs, 5, 30, 0.1, s0, np.random.default_rng(1))
    rp.update_externals(reference_path=ref, x_0=x0, desired_velocity=12.0, predictions=preds)
    return rp


def candidate_values(step, g) -> dict:
    """one candidate through the step's single-sample read path while the step is fresh (a throw-away read: nothing is cached
    in a sample)"""
    p = step.engine.sample(g, step.agent)
    lon, lat, tl, tau = step.engine.coeffs(g, step.agent)
    return dict(planes=np.array(p), lon=np.array(lon), lat=np.array(lat), tl=tl, tau=tau, raw=np.array(step.engine.costmap(step.agent)[g]))


def sample_values(t) -> dict:
    c, cl = t.cartesian, t.curvilinear
    planes = np.stack([getattr(c, n) for n in CART] + [getattr(cl, n) for n, _ in CURV])
    return dict(planes=planes, lon=np.array(t.trajectory_long.coeffs), lat=np.array(t.trajectory_lat.coeffs), tl=t.actual_traj_length,
                tau=t.trajectory_lat.delta_tau, raw=np.array([t.costMap[n][0] for n in t._step.inputs.cost_names]))


def same_values(a, b):
    for k in a:
        x, y = np.ascontiguousarray(a[k], np.float64), np.ascontiguousarray(b[k], np.float64)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)), k


def planner_route(engine):
    rp = make_planner(engine)
    try:
        pair = rp.plan()
        assert pair is not None
        step1 = rp.last_step
        old_list = rp.all_traj
        kept = [old_list[j] for j in (1, 7, 40, 200)]
        assert all(t is not rp.optimal_trajectory for t in kept)
        want = [candidate_values(step1, t.uniqueId) for t in kept]
        cart, cl, lon, lat = pair
        rp.update_externals(x_0=cart[1], x_cl=(lon[1], lat[1]), desired_velocity=11.0)
        assert rp.plan() is not None and rp.last_step is not step1 and step1._stale
        for t, w in zip(kept, want):
            same_values(sample_values(t), w)
        assert not np.array_equal(rp.last_step.sample(kept[0].uniqueId).cartesian.x, kept[0].cartesian.x)
        # the stale list keeps serving the rescued entries; a j nobody held before the next step stays an error
        assert old_list is not rp.all_traj and old_list[7] is kept[1] and len(old_list) == len(step1.sorted_ids())
        same_values(sample_values(old_list[40]), want[2])
        with pytest.raises(RuntimeError, match=STALE):
            old_list[3].cartesian
    finally:
        rp.close()


def escalation_route(engine):
    """nothing acceptable at level 2 -> level 3 inside ONE plan(): samples an occlusion module took at level 2 read level-2
    values afterwards"""
    rp = make_planner(engine, sampling_min=2, sampling_max=4)
    taken = []

    class Module:   # an occlusion module that looks at the set and keeps three of its samples (planner.py:329-392)
        def calc_costs(self, trajs):
            if not taken:
                step = trajs[0]._step
                taken.extend((t, candidate_values(step, t.uniqueId)) for t in trajs[:3])

        def trajectory_safety_assessment(self, traj):
            return None, traj._step is not taken[0][0]._step   # nothing of the first level passes

    try:
        rp.occlusion_module, rp.use_occ_model = Module(), True
        rp.plan()
        assert len(taken) == 3 and taken[0][0]._step is not rp.last_step and taken[0][0]._step._stale
        assert rp.last_step.inputs.n_candidates > taken[0][0]._step.inputs.n_candidates
        for t, w in taken:
            same_values(sample_values(t), w)
    finally:
        rp.close()


def test_planner_samples_survive_the_next_plan():
    planner_route(PackagingOracleEngine())
    planner_route(OracleEngine())


def test_planner_samples_survive_a_level_escalation():
    escalation_route(PackagingOracleEngine())


@pytest.mark.gpu
def test_planner_samples_survive_the_next_plan_gpu():
    planner_route(None)


@pytest.mark.gpu
def test_planner_samples_survive_a_level_escalation_gpu():
    escalation_route(None)


# ------------------------------------------------------------------------------------------------ what was written to a sample
def test_fields_written_to_samples_stay_with_the_candidate():
    """the host walk writes boundary_harm / _coll_detected onto the survivors it rejects and drops them; step.sample(), all_traj and
    the logger's bulk view read them back (planner.py:381-382; logging_formats._BulkStep) -- as on a step that pinned its samples"""
    from frenetix_motion_planner_amd.logging_formats import _BulkStep
    rp = make_planner(PackagingOracleEngine())
    rejected = []

    def check(traj):
        if len(rejected) < 3:
            rejected.append(traj.uniqueId)
            return 0.7
        return 0

    rp.road_boundary_check = check
    assert rp.plan() is not None
    step = rp.last_step
    gc.collect()
    assert len(rejected) == 3 and rp.optimal_trajectory.uniqueId not in rejected
    assert not {t.uniqueId for t in step.live_samples()} & set(rejected)        # nobody holds them ...
    for g in rejected:                                                          # ... and what was written is still the candidate's
        t = step.sample(g)
        assert t.boundary_harm == 0.7 and t._coll_detected is False
    assert rp.optimal_trajectory.boundary_harm == 0 and rp.optimal_trajectory._coll_detected is False
    by_id = {t.uniqueId: t for t in rp.all_traj}
    assert [by_id[g].boundary_harm for g in rejected] == [0.7, 0.7, 0.7]
    gc.collect()
    bulk = _BulkStep(step, np.asarray(rp.all_traj._order(), dtype=np.int64))
    harm = {t.uniqueId: (t.boundary_harm, t._coll_detected) for t in bulk.samples}
    assert all(harm[g] == (0.7, False) for g in rejected)
    # write, drop, read again through all_traj -- every writable field, and one the package does not know
    t = rp.all_traj[5]
    g = t.uniqueId
    t._ego_risk, t._obst_risk, t.cost, t.valid, t.harm_occ_module, t.note = 0.25, 0.5, t.cost + 1.0, False, 0.1, "seen"
    c = t.cost
    del t, by_id, bulk
    gc.collect()
    assert g not in {x.uniqueId for x in step.live_samples()}
    t = rp.all_traj[5]     # (the list's order was fixed before the write)
    assert t.uniqueId == g and (t._ego_risk, t._obst_risk, t.cost, t.valid, t.harm_occ_module, t.note) == (0.25, 0.5, c, False, 0.1, "seen")
    # ... and with the batch of samples the occlusion walk and the adapter's list create at once
    del t
    gc.collect()
    many = {x.uniqueId: x for x in step.samples(range(40))}
    if g in many:
        assert many[g]._ego_risk == 0.25
    for r in rejected:
        if r in many:
            assert many[r].boundary_harm == 0.7
    # written state does not make a sample "held": nothing of it is rescued
    cart, cl, lon, lat = rp.trajectory_pair
    del many
    gc.collect()
    rp.update_externals(x_0=cart[1], x_cl=(lon[1], lat[1]), desired_velocity=11.0)
    rp.plan()
    assert step._stale and step._snap is None
    assert step.sample(g)._ego_risk == 0.25        # (still the candidate's; its device data is gone)
    with pytest.raises(RuntimeError, match=STALE):
        step.sample(g).cartesian


def test_planner_retain_samples_off():
    rp = make_planner(PackagingOracleEngine(), retain_samples=False)
    pair = rp.plan()
    kept = rp.all_traj[5]
    best = rp.optimal_trajectory
    cart, cl, lon, lat = pair
    rp.update_externals(x_0=cart[1], x_cl=(lon[1], lat[1]), desired_velocity=11.0)
    rp.plan()
    with pytest.raises(RuntimeError, match=STALE):
        kept.cartesian
    assert best.cartesian.x.shape == (31,)   # the chosen trajectory is materialised, as before


# ------------------------------------------------------------------------------------------------ launch first, consume second
class RegistryOracle(StepRegistry, PackagingOracleEngine):
    """a stand-in on the registry mix-in: rescues before it overwrites, as FrenetEngine does"""

    def plan_batch(self, inps):
        if self._steps:
            self.rescue_steps()
        return super().plan_batch(inps)


def batch_like_step(rp, engine):
    """AgentBatchHip.step for one planner: the batch is launched FIRST, plan_consume comes second (multiagent.py)"""
    inp = rp.plan_begin()
    res, pk = engine.plan_batch_packaged([inp], [rp.x_0.yaw_rate])
    best = rp.plan_consume(inp, res[0], engine, 0, package=pk[0])
    return rp.plan_finish(best, 0.0)


def overwrite_rule(engine):
    rp = make_planner(engine)
    engine.set_package(True)
    pair = batch_like_step(rp, engine)
    step1 = rp.last_step
    kept = [rp.all_traj[j] for j in (2, 9, 77)]
    want = [candidate_values(step1, t.uniqueId) for t in kept]
    cart, cl, lon, lat = pair
    rp.update_externals(x_0=cart[1], x_cl=(lon[1], lat[1]), desired_velocity=11.0)
    batch_like_step(rp, engine)
    assert rp.last_step is not step1
    new = candidate_values(rp.last_step, kept[0].uniqueId)
    assert not np.array_equal(new["planes"], want[0]["planes"])
    return kept, want


def test_engine_rescues_before_it_overwrites():
    kept, want = overwrite_rule(RegistryOracle())
    for t, w in zip(kept, want):
        same_values(sample_values(t), w)


def test_without_the_registry_a_late_invalidate_raises_and_never_reads_the_new_step():
    kept, _ = overwrite_rule(PackagingOracleEngine())
    for t in kept:
        with pytest.raises(RuntimeError, match=STALE):
            t.cartesian
        with pytest.raises(RuntimeError, match=STALE):
            t.costMap


@pytest.mark.gpu
def test_agent_batch_keeps_samples_across_a_batched_step():
    """three agents on one engine context: four samples of agent 1's all_traj, the batch steps again (different ego states).
    With the rescue in the wrong place this returns the new step's numbers, not an error."""
    import os
    from frenetix_motion_planner_amd import commonroad_xml as crx
    from frenetix_motion_planner_amd import multiagent
    sc = crx.read_scenario_json(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ZAM_Tjunction-1_42_T-1.scenario.json"))
    sim = multiagent.MultiAgentSimulation(sc, number_of_agents=2, pipeline_groups=1)
    try:
        assert len(sim.batch.agents) == 3 and len(sim.batch.engines) == 1
        sim.step()
        rp = sim.batch.agents[1].planner
        step1 = rp.last_step
        assert step1 is not None and step1.agent == 1 and step1.engine is sim.batch.engine
        kept = [rp.all_traj[j] for j in (1, 5, 30, 120)]
        want = [candidate_values(step1, t.uniqueId) for t in kept]
        launches = sim.batch.launches
        for _ in range(3):
            sim.step()
        assert sim.batch.launches == launches + 1 and rp.last_step is not step1 and step1._stale
        assert rp.last_step.engine is sim.batch.engine
        new = candidate_values(rp.last_step, kept[0].uniqueId)
        assert not np.array_equal(new["planes"], want[0]["planes"])
        for t, w in zip(kept, want):
            same_values(sample_values(t), w)
    finally:
        sim.close()


@pytest.mark.gpu
def test_engine_close_rescues_kept_samples():
    h, matrix = make_handler(None)
    twin, _ = make_handler(None)
    for hh in (h, twin):
        hh.reset_Trajectories()
        evaluate(hh, matrix())
    kept = h.get_sorted_trajectories()[10:14]
    before = [read_all(t) for t in twin.get_sorted_trajectories()[10:14]]
    twin.engine.close()
    h.engine.close()
    for t, b in zip(kept, before):
        same_bits(read_all(t), b)


@pytest.mark.gpu
def test_rescued_sample_of_a_select_only_step_still_says_not_ready():
    """a rescued sample answers as it would have on the fresh step -- also for what the step did not produce"""
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from frenetix_motion_planner_amd.trajectories import PlanStepResult
    kw = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(5, 7, 9), n_obstacles=3)
    inp = synthetic.make_inputs(write_bundle=False, write_costmap=False, **kw)
    with FrenetEngine(max_candidates=4096) as eng:
        step = PlanStepResult(eng, inp, eng.plan_step(inp))
        cost, flags = eng.costs()
        fresh, kept = step.sample(3), step.sample(5)
        with pytest.raises(ValueError, match="FX_MODE_WRITE_BUNDLE"):
            fresh.cartesian
        with pytest.raises(ValueError, match="FX_MODE_WRITE_COSTMAP"):
            fresh.costMap
        del fresh
        eng.plan_step(synthetic.make_inputs(**kw))       # the engine rescues `kept` before it overwrites
        assert step._stale and step._snap_ids.tolist() == [5] and step._snap["planes"] is None
        with pytest.raises(ValueError, match="FX_MODE_WRITE_BUNDLE"):
            kept.cartesian
        with pytest.raises(ValueError, match="FX_MODE_WRITE_BUNDLE"):
            kept.trajectory_long
        with pytest.raises(ValueError, match="FX_MODE_WRITE_COSTMAP"):
            kept.costMap
        assert kept.cost == cost[5] and kept._flags == int(flags[5])
        with pytest.raises(RuntimeError, match=STALE):
            step.sample(7)
