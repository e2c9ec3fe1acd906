"""The planner's risk-cost paths on `blocked_planner` (every feasible candidate collides):
set_risk_cost_weights + set_fallback_selector("min_risk_cost") picks the restatement's arg-min of the weighted total in both
responsibility modes; risk_costs() without a model and on a select-only step raises."""
import numpy as np
import pytest

from tests import risk_costs_restatement as rcr
from tests.test_planner_host import blocked_planner
from tests.test_risk_planner import HARM, MASS, RISK, _with_model
from frenetix_motion_planner_amd import _abi

pytestmark = pytest.mark.gpu

WEIGHTS = dict(bayes=1.0, equality=0.5, maximin=2.0, ego=0.25, responsibility=1.5)


def _reach_set(rp):
    """a reach set of the wall on the lane ahead: the left half of the road at 1 s, so that some candidates' points lie inside"""
    poly = np.array([[20.0, 0.35], [60.0, 0.35], [60.0, 9.0], [40.0, 12.0], [20.0, 9.0]])
    big = np.array([[-1e3, -1e3], [1e3, -1e3], [1e3, 1e3], [-1e3, 1e3]])
    import types
    return types.SimpleNamespace(reach_sets={rp.x_0.time_step: {5: [{0.0: big}, {0.3: poly[:4]}, {1.0: poly}]}})


@pytest.mark.parametrize("mode", ["action_space", "reach_set"])
def test_min_risk_cost_fallback_picks_the_restated_arg_min(mode):
    rp = _with_model(sampling_min=1, sampling_max=3)
    with pytest.raises(ValueError):
        rp.set_fallback_selector("min_risk_cost")   # no weights yet
    rp.set_risk_cost_weights(WEIGHTS, responsibility_mode=mode)
    rp.set_reach_set(_reach_set(rp))
    rp.set_fallback_selector("min_risk_cost")
    pair = rp.plan()
    step, best = rp.last_step, rp.optimal_trajectory
    assert step.result["best_index"] == -1 and pair is not None and best is not None
    ids = np.nonzero(step.mask(_abi.FX_FLAG_VALID) & step.mask(_abi.FX_FLAG_FEASIBLE) & step.mask(_abi.FX_FLAG_RETURNED))[0]
    cart = [step.sample(int(g)).cartesian for g in ids]
    P = [np.array([getattr(c, n) for c in cart]) for n in ("x", "y", "theta", "v")]
    d = rcr.calc_risk_detail(*P, rp.predictions, {5: "car"}, RISK, HARM, rp.vehicle_params.length, rp.vehicle_params.width, MASS)
    assert np.count_nonzero(d["ego_risk"]) > len(ids) // 2
    if mode == "action_space":
        resp = [rcr.responsibility_action_space(d["obst_risk_max"][c], rp.predictions, rp.x_0.position, rp.x_0.orientation)
                for c in range(len(ids))]
    else:
        sets = rp.reach_set.reach_sets[rp.x_0.time_step]
        rs = [rcr.responsibility_reach_set(P[0][c], P[1][c], rp.dT, sets, d["obst_risk_max"][c], [5]) for c in range(len(ids))]
        resp = [r[0] for r in rs]
        inside = np.array([r[1][0][1:].any() for r in rs])
        assert inside.any() and not inside.all()
    want = rcr.costs(d, 0.0, list(WEIGHTS.values()), resp)
    s = np.sort(want["total"])
    assert s[1] - s[0] > 1e-9, "near tie for the minimum"
    assert best.uniqueId == rcr.argmin_index(want["total"], ids)
    got = rp.risk_costs(ids)
    assert got["min_cost_index"] == best.uniqueId
    # K = 1: sums of 2K + 1 values 3e-12, maximin 10e-12 (test_risk_costs_gpu.py), weighted
    w = WEIGHTS
    bound = (w["bayes"] + w["equality"] + w["ego"] + w["responsibility"]) * 3e-12 + w["maximin"] * 10e-12
    assert np.abs(got["total"] - want["total"]).max() <= bound * max(1.0, np.abs(want["total"]).max())


def test_risk_costs_needs_the_model_and_the_bundle():
    from frenetix_motion_planner_amd import synthetic, risk
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    rp = blocked_planner(engine=None, emergency_selection=True)
    rp.plan()
    with pytest.raises(ValueError):
        rp.risk_costs()
    with pytest.raises(ValueError):
        rp.set_risk_cost_weights(WEIGHTS, responsibility_mode="reachset")
    # a select-only step (no materialised bundle) raises as risk() does
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, grid=(3, 5, 5), n_obstacles=2, write_bundle=False)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
        params = risk.risk_params(RISK, HARM, 4.5, 1.6, MASS)
        with pytest.raises(ValueError):
            eng.risk(params)
        with pytest.raises(ValueError):
            eng.risk_detail(params)
        with pytest.raises(ValueError):
            eng.risk_costs(params, risk.risk_cost_params(list(WEIGHTS.values())))
