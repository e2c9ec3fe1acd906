"""cost_weights["responsibility"] in ReactivePlannerHip: the pass beside the step runs per sampling level
and its totals, order, winner, cost-map entry and risk fields are what the planner hands out.  The host side of the comparison is
the restatement of get_responsibility_cost (tests/risk_costs_restatement.py) on the step's own read-back planes, re-summed as
tests/test_responsibility_cost_gpu.py does.  The checks without a GPU: the configuration errors, and that weight sets without the
term give the plan step the names, ids and weights they always gave it and the logs the text they always gave them."""
import types

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import risk_costs_restatement as rcr
from tests.test_planner_host import blocked_planner

W = 0.5
TYPES = {5: "car", 6: "car"}


def _planner(mode="reach_set", reach=True, **cfg):
    """the blocked planner with a short wall beside the lane (some selectable candidates collide with it, most do not), the risk
    model, a reach set of the wall over the left half of the road, and the responsibility term weighted"""
    from tests.test_risk_planner import HARM, MASS, RISK
    rp = blocked_planner(engine=None, responsibility_mode=mode, **cfg)
    n = 31
    wall = dict(rp.predictions[5], shape=dict(length=1.0, width=3.0), pos_list=np.tile([[27.0, 2.0]], (n, 1)), v_list=np.full(n, 0.5))
    preds = {5: wall}
    if mode == "action_space":
        # the wall lies inside the ego's +-pi/4 view, where the action-space rule assigns no responsibility: a long vehicle
        # behind and beside the ego, two metres clear of its footprint, whose front centre is within the 5 m gate of the first steps
        preds[6] = dict(pos_list=np.tile([[15.0, 4.0]], (n, 1)), cov_list=np.tile(np.eye(2) * 0.4, (n, 1, 1)), orientation_list=np.zeros(n),
                        v_list=np.full(n, 3.0), shape=dict(length=8.0, width=1.8))
    rp.update_externals(predictions=preds)
    rp.set_risk_model(RISK, HARM, {k: "car" for k in preds}, MASS)
    if reach:
        poly = np.array([[20.0, 0.35], [60.0, 0.35], [60.0, 9.0], [40.0, 12.0], [20.0, 9.0]])
        big = np.array([[-1e3, -1e3], [1e3, -1e3], [1e3, 1e3], [-1e3, 1e3]])
        rp.set_reach_set(types.SimpleNamespace(reach_sets={rp.x_0.time_step: {5: [{0.0: big}, {0.3: poly[:4]}, {1.0: poly}]}}))
    rp.set_cost_function(dict(rp.cost_weights, responsibility=W))
    return rp


def _restated(rp, step, mode, pred=None):
    """(costed ids, resp, total, flags) of a step on the host"""
    from tests.test_responsibility_cost_gpu import _resum
    from tests.test_risk_planner import HARM, MASS, RISK
    eng, inp = step.engine, step.inputs
    _, flags = eng.costs(step.agent)
    ids = np.nonzero(flags & _abi.FX_FLAG_COSTED)[0]
    P = [eng.plane(n, step.agent).T[ids] for n in ("x", "y", "theta", "v")]
    v = rp.vehicle_params
    d = rcr.calc_risk_detail(*P, rp.predictions, TYPES, RISK, HARM, v.length, v.width, MASS)
    if mode == "action_space":
        resp = [rcr.responsibility_action_space(d["obst_risk_max"][c], rp.predictions, rp.x_0.position, rp.x_0.orientation) for c in range(len(ids))]
    else:
        sets = rp.reach_set.reach_sets[rp.x_0.time_step]
        resp = [rcr.responsibility_reach_set(P[0][c], P[1][c], rp.dT, sets, d["obst_risk_max"][c], [5])[0] for c in range(len(ids))]
    resp = np.asarray(resp, np.float64)
    deferred = bool(eng.step_info()["obstacle_kernel"])
    total = _resum(eng.costmap(step.agent)[ids], np.asarray(inp._cost_w), list(inp.cost_names), W, resp, deferred,
                   pred=None if pred is None else pred[ids])
    return ids, resp, total, flags, d


def _free(order, flags):
    return [g for g in order if (flags[g] & _abi.FX_FLAG_SELECTABLE) and not (flags[g] & (_abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY))]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["reach_set", "action_space"])
def test_planner_plans_with_the_term(mode):
    rp = _planner(mode)
    pair = rp.plan()
    step, best = rp.last_step, rp.optimal_trajectory
    assert pair is not None and best is not None and step._override is not None
    assert "responsibility" not in step.inputs.cost_names
    ids, resp, total, flags, d = _restated(rp, step, mode)
    assert (resp != 0).sum() > len(ids) // 8
    order = ids[np.argsort(total, kind="stable")]
    free = _free(order, flags)
    assert free and (flags[ids] & _abi.FX_FLAG_COLLISION).any()
    key = dict(zip(ids.tolist(), total.tolist()))
    # two totals closer than device and restatement agree may swap, nothing else: resp agrees to 5e-12 (K <= 2: 2K + 1 values)
    assert best.uniqueId == free[0] or abs(key[best.uniqueId] - key[free[0]]) <= W * 5e-12 * max(abs(key[free[0]]), 1.0)
    assert np.abs(step.cost[ids] - total).max() <= W * 5e-12 * max(1.0, np.abs(total).max())
    # the sorted list follows the override
    trajs = step.sorted_trajectories()
    got = np.array([t.uniqueId for t in trajs])
    assert np.array_equal(got, ids[np.argsort(step.cost[ids], kind="stable")])
    e, o, _ = step.engine.risk(rp._risk_model["params"], ids)
    for t in trajs[:40]:
        g = t.uniqueId
        k = int(np.searchsorted(ids, g))
        raw, weighted = t.costMap["responsibility"]
        assert abs(raw - resp[k]) <= 5e-12 and weighted == W * raw and t.cost == step.cost[g]
        assert t._ego_risk == e[k] and t._obst_risk == o[k]
    # held samples keep all of it past the next step
    held = trajs[3]
    keep = (held.uniqueId, held.cost, held.costMap["responsibility"], held._ego_risk, held._obst_risk)
    del trajs
    rp.plan()
    assert rp.last_step is not step
    assert keep == (held.uniqueId, held.cost, held.costMap["responsibility"], held._ego_risk, held._obst_risk)
    again = step.sample(int(ids[0]))   # (a new view of the old step answers from the pass as well)
    assert again._ego_risk == e[0] and again._obst_risk == o[0]


@pytest.mark.gpu
def test_without_a_reach_set_the_term_is_zero():
    rp = _planner("reach_set", reach=False)
    rp.plan()
    step = rp.last_step
    assert step._override is None   # (upstream's condition: no pass runs)
    own, _ = step.engine.costs()
    assert np.array_equal(step.cost, own)
    assert rp.optimal_trajectory.costMap["responsibility"] == (0.0, 0.0) and step.sample(0).costMap["responsibility"] == (0.0, 0.0)
    ref = blocked_planner(engine=None)
    ref.update_externals(predictions=rp.predictions)
    ref.plan()
    assert np.array_equal(ref.last_step.cost, step.cost, equal_nan=True)
    assert ref.optimal_trajectory.uniqueId == rp.optimal_trajectory.uniqueId


@pytest.mark.gpu
def test_composes_with_the_collision_probability():
    rp = _planner("action_space", prediction_cost="collision_probability")
    assert rp.plan() is not None
    step, best = rp.last_step, rp.optimal_trajectory
    v = rp.vehicle_params
    prob = step.engine.prediction_probability(v.length, v.width)["prob"]
    ids, resp, total, flags, d = _restated(rp, step, "action_space", pred=prob)
    assert (prob[ids] > 0).sum() > len(ids) // 4
    assert np.abs(step.cost[ids] - total).max() <= W * 5e-12 * max(1.0, np.abs(total).max())
    free = _free(ids[np.argsort(step.cost[ids], kind="stable")], flags)
    assert best.uniqueId == free[0]
    cm = best.costMap
    assert cm["prediction"][0] == prob[best.uniqueId] and "responsibility" in cm


def test_configuration_errors():
    from tests.test_risk_planner import HARM, MASS, RISK
    rp = blocked_planner()
    weights = dict(rp.cost_weights, responsibility=W)
    with pytest.raises(ValueError, match="set_risk_model"):
        rp.set_cost_function(weights)
    with pytest.raises(ValueError, match="set_risk_model"):
        rp.plan()
    rp = blocked_planner(sparse_bundle_k=8)
    rp.set_risk_model(RISK, HARM, {5: "car"}, MASS)
    with pytest.raises(ValueError, match="bundle"):
        rp.set_cost_function(weights)
    rp = blocked_planner(responsibility_mode="reachset")
    rp.set_risk_model(RISK, HARM, {5: "car"}, MASS)
    with pytest.raises(ValueError, match="responsibility_mode"):
        rp.set_cost_function(weights)
    rp = blocked_planner()
    rp.set_cost_function(dict(rp.cost_weights, responsibility=0.0))   # (a zero weight asks for nothing)


def test_the_plan_step_never_sees_the_term():
    """the weights the planner hands the plan step are the ones of the weight set without the term -- names, ids and weights
    equal -- and PlanInputs goes on refusing what the hot path does not compute, `velocity` among it"""
    from frenetix_motion_planner_amd import synthetic
    from tests.test_risk_planner import HARM, MASS, RISK
    seen = []
    for extra in ({}, dict(responsibility=W)):
        rp = blocked_planner()
        rp.set_risk_model(RISK, HARM, {5: "car"}, MASS)
        rp.set_cost_function(dict(rp.cost_weights, **extra))
        rp.plan()
        inp = rp.last_step.inputs
        seen.append((list(inp.cost_names), inp._cost_id.tolist(), inp._cost_w.tolist(), dict(inp.cost_weights)))
    assert seen[0] == seen[1] and "responsibility" not in seen[1][0] and len(seen[0][0]) > 3
    with pytest.raises(NotImplementedError):
        synthetic.make_inputs(ref_kind="arc", grid=(2, 2, 2), cost_weights=dict(lateral_jerk=0.2, velocity=1.0))


# ---- the logs (logging_formats.py) ----
def _logged_planner(tmp_path=None):
    """a planner on the CPU stand-in engine that keeps every trajectory of its step for the logs"""
    from frenetix_motion_planner_amd import VehicleParams, synthetic
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig, ReactivePlannerHip, ReactivePlannerState
    from tests.oracle_engine import OracleEngine
    ref = synthetic.reference_polyline("arc", 400, 0.5, 0.01)
    cs = synthetic.CoordinateSystem(ref)
    s0 = float(cs.ref_pos[40]) + 0.1
    x0 = ReactivePlannerState(time_step=7, position=cs.convert_to_cartesian_coords(s0, 0.2), orientation=float(cs.ref_theta[40]), velocity=9.0)
    preds = synthetic.synthetic_predictions(cs, 3, 30, 0.1, s0, np.random.default_rng(5))
    rp = ReactivePlannerHip(PlannerConfig(save_all_traj=True, sampling_min=1, sampling_max=2), VehicleParams(), engine=OracleEngine())
    rp.update_externals(reference_path=ref, x_0=x0, desired_velocity=11.0, predictions=preds)
    assert rp.plan() is not None
    return rp


def _write_logs(path, step, trajs, cost_params):
    """every file of the loggers for one step: all trajectories and the logs.csv line of the step's best"""
    from frenetix_motion_planner_amd import logging_formats as lf
    from tests.test_logging_formats import gen
    lg = lf.DataLoggingCosts(str(path), save_all_traj=True, cost_params=cost_params)
    lg.log_all_trajectories(trajs, 7)
    lg.log(step.best, 7, [0] * 11, 50.0, 0.01, [type("S", (), {"position": np.array([1.0, 2.0])})()], desired_velocity=11.0)
    lg.close()
    return gen.dump(str(path))


def _cost_columns(dump):
    """trajectories.csv of a dump: (names of the cost columns, {unique id: (total, [a value per cost column])})"""
    import json
    lines = dump["files"]["trajectories.csv"].splitlines()
    head = lines[0].split(";")
    first = head.index("costs_cumulative_weighted")
    cols = [k for k, h in enumerate(head) if h.endswith("_cost")]
    assert cols == list(range(first + 1, first + 1 + len(cols)))
    rows = {}
    for ln in lines[1:]:
        f = ln.split(";")
        rows[int(f[2])] = (float(json.loads(f[first])), [float(json.loads(f[k])) for k in cols])
    return [head[k][:-len("_cost")] for k in cols], rows


def test_logs_of_a_weight_set_without_the_term_are_unchanged(tmp_path):
    """What the plane-wise log of a whole step is formatted from -- names, raw costs and weights -- is, for a weight set without
    the term, the step's cost names, its cost map and its weights in every bit, as before the term existed; the rest of
    logging_formats.py formats them as it did.  So the files are the earlier ones byte for byte: no column for the term in
    logs.csv, trajectories.csv or the costs table, and the plane-wise path still writes what the per-trajectory path writes
    (a wall-clock time is the only field of logs.csv that is not the step's; it is given here)."""
    from frenetix_motion_planner_amd.reactive_planner import _LazySortedList
    rp = _logged_planner()
    step, inp = rp.last_step, rp.last_step.inputs
    lazy = _LazySortedList(step)
    ids = np.asarray(lazy._order(), np.int64)
    assert len(ids) > 50 and step._override is None and step._extras == {}
    names, raw, weights = step.cost_columns(ids)
    own = step.engine.costmap(step.agent)[ids]
    assert names == list(inp.cost_names) and len(names) > 3
    assert raw.dtype == own.dtype == np.float64 and raw.tobytes() == np.ascontiguousarray(own).tobytes()
    want_w = np.array([inp.cost_weights[n] for n in names])
    assert weights.dtype == want_w.dtype and weights.tobytes() == want_w.tobytes()
    outs = [_write_logs(tmp_path / str(k), step, trajs, dict(rp.cost_weights)) for k, trajs in enumerate((lazy, list(lazy)))]
    assert outs[0] == outs[1]
    for f in ("logs.csv", "trajectories.csv"):
        assert "responsibility" not in outs[0]["files"][f]
    assert not any("responsibility" in str(r) for r in outs[0]["schema"])
    logged, rows = _cost_columns(outs[0])
    assert logged == sorted(rp.cost_weights) and len(rows) == len(ids)
    k = [logged.index(n) for n in names]
    for j, g in enumerate(ids):   # (the weighted values of the step's own terms, and 0 for a name the step does not compute)
        assert rows[int(g)][0] == step.cost[g] and [rows[int(g)][1][c] for c in k] == [float(weights[c] * raw[j, c]) for c in range(len(names))]
        assert sum(rows[int(g)][1]) == sum(rows[int(g)][1][c] for c in k)


def test_the_weighted_term_is_a_column_of_the_logs(tmp_path):
    """With the term installed beside the step (here by hand, on the CPU stand-in: a raw value per candidate and the total
    re-summed with it in the logged order), the plane-wise log of all trajectories has the term's column: it equals
    costMap["responsibility"][1], the row's columns add up to the row's total, and the per-trajectory path writes the same files."""
    from frenetix_motion_planner_amd.reactive_planner import _LazySortedList
    from frenetix_motion_planner_amd.trajectories import PlanStepResult
    rp = _logged_planner()
    last = rp.last_step   # (a new view of the step: the override goes in before samples are handed out, as the planner does it)
    step, inp = PlanStepResult(last.engine, last.inputs, last.result, last.agent), last.inputs
    own, flags = step.engine.costs(step.agent)
    costed = np.nonzero(flags & _abi.FX_FLAG_COSTED)[0]
    resp = np.random.default_rng(11).uniform(0.0, 2.0, len(own))
    resp[costed[::3]] = 0.0
    names = sorted(list(inp.cost_names) + ["responsibility"])
    cm = step.engine.costmap(step.agent)
    total = np.zeros(len(own))
    for n in names:   # (the sum the columns are checked against: left to right in the logged order)
        total = total + (W * resp if n == "responsibility" else float(inp.cost_weights[n]) * cm[:, list(inp.cost_names).index(n)])
    step.set_cost_override(total, np.full(len(own), np.nan), int(costed[np.argmin(total[costed])]), extras={"responsibility": (resp, W)})
    lazy = _LazySortedList(step)
    params = dict(rp.cost_weights, responsibility=W)
    outs = [_write_logs(tmp_path / str(k), step, trajs, params) for k, trajs in enumerate((lazy, list(lazy)))]
    assert outs[0] == outs[1]
    logged, rows = _cost_columns(outs[0])
    assert logged == sorted(params) and len(rows) == len(costed) > 50
    c = logged.index("responsibility")
    sql = {r[1]: r for r in outs[0]["tables"]["costs"]}
    for g in costed:
        t = step.sample(int(g))
        tot, cols = rows[int(g)]
        assert cols[c] == t.costMap["responsibility"][1] == W * resp[g] and tot == t.cost == total[g]
        acc = 0.0
        for v in cols:
            acc = acc + v
        assert acc == tot
        assert sql[int(g)][2] == tot and sql[int(g)][3 + c] == cols[c]
    assert sum(rows[int(g)][1][c] != 0 for g in costed) > len(costed) // 2


@pytest.mark.gpu
def test_the_planner_logs_the_term(tmp_path):
    """the planner's own log of all trajectories with the term weighted: the column is costMap["responsibility"][1] of the pass,
    not 0, and the columns of a row add up to its total -- to the rounding of a sum of n <= 13 doubles taken in another order
    (the step sums its tail terms apart): n * 2^-53 * sum |terms| per sum, twice that between the two."""
    import json
    from frenetix_motion_planner_amd import logging_formats as lf
    from tests.test_logging_formats import gen
    rp = _planner("reach_set", save_all_traj=True)
    params = dict(rp.cost_weights)
    rp.logger = lf.DataLoggingCosts(str(tmp_path), save_all_traj=True, cost_params=params)
    assert rp.plan() is not None
    rp.logger.close()
    step = rp.last_step
    logged, rows = _cost_columns(gen.dump(str(tmp_path)))
    assert logged == sorted(params)
    c = logged.index("responsibility")
    nz = 0
    for g, (tot, cols) in rows.items():
        t = step.sample(g)
        assert cols[c] == t.costMap["responsibility"][1] and tot == t.cost == step.cost[g]
        assert abs(sum(cols) - tot) <= 2 * 13 * 2.0 ** -53 * sum(abs(v) for v in cols)
        nz += cols[c] != 0
    assert len(rows) > 50 and nz > len(rows) // 8
    line = open(tmp_path / "logs.csv").read().splitlines()
    head, last = line[0].split(";"), line[-1].split(";")
    assert float(json.loads(last[head.index("responsibility_cost")])) == rp.optimal_trajectory.costMap["responsibility"][1]
