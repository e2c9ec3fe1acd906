"""The collision probability as the prediction cost through the frenetix route and the planner: the
handler of tests/handler_fixture.py with prediction_cost="collision_probability" hands out the pass's order, costs and cost-map
entries, and leaves the default route as it is; ReactivePlannerHip walks the restated order."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import predprob_restatement as pp
from tests.handler_fixture import evaluate, make_handler
from tests.test_planner_host import blocked_planner

pytestmark = pytest.mark.gpu


def _restated(step, preds, length, width):
    """(costed ids, prob, total) of a step: the restatement on the step's own read-back planes, re-summed with its raw cost rows"""
    eng, inp = step.engine, step.inputs
    _, flags = eng.costs(step.agent)
    ids = np.nonzero(flags & _abi.FX_FLAG_COSTED)[0]
    x, y, th = (eng.plane(n, step.agent).T[ids] for n in ("x", "y", "theta"))
    prob, _, _ = pp.prediction_probability(x, y, th, preds or {}, length, width)
    n_pred = inp.cost_names.index("prediction")
    total = pp.resum(eng.costmap(step.agent)[ids], inp._cost_w, n_pred, prob)
    return ids, prob, total, flags


def test_handler_hands_out_the_pass():
    h, matrix = make_handler()
    h.prediction_cost = "collision_probability"
    m = matrix()
    evaluate(h, m)
    step = h._step
    pc = h._costs["prediction"]
    ids, prob, total, flags = _restated(step, h._predictions(), pc.length, pc.width)
    assert len(ids) > 100 and (prob > 0).sum() > 0
    trajs = h.get_sorted_trajectories()
    # the stable argsort of the restated totals: the device's totals agree with them to the last bits that decide the order
    dev = step.engine.prediction_probability(pc.length, pc.width)
    assert np.abs(dev["prob"][ids] - prob).max() <= (len(h._predictions()) * 30 + 1) * 1e-12
    want = ids[np.argsort(total, kind="stable")]
    got = np.array([t.uniqueId for t in trajs])
    assert sorted(got) == sorted(want)
    if not np.array_equal(got, want):
        # two totals closer than device and restatement agree may swap, nothing else: the probabilities agree to 1e-12 per term
        # (asserted above at the sum), measured 1e-14, and enter the total with the weight 0.2
        key = dict(zip(ids.tolist(), total.tolist()))
        assert all(abs(key[a] - key[b]) <= 1e-12 * max(abs(key[a]), 1.0) for a, b in zip(got.tolist(), want.tolist()))
    assert np.array_equal(got, ids[np.argsort(dev["total"][ids], kind="stable")])
    w = pc.weight
    assert len(trajs) == len(ids)
    for t in trajs:
        g = t.uniqueId
        assert t.cost == dev["total"][g]
        raw, weighted = t.costMap["prediction"]
        assert raw == dev["prob"][g] and weighted == w * dev["prob"][g]
    assert step.best is None or step.best.uniqueId == dev["best_index"]
    # a held sample survives reset_Trajectories() with those values
    held = trajs[3]
    g, c = held.uniqueId, held.cost
    del trajs
    h.reset_Trajectories()
    evaluate(h, matrix(ds0=0.5))
    assert held.cost == c == dev["total"][g] and held.costMap["prediction"][0] == dev["prob"][g]
    assert held.cartesian.x.shape == (31,)


def test_default_handler_is_unchanged():
    a, matrix = make_handler()
    b, _ = make_handler()
    assert a.prediction_cost == "inverse_mahalanobis"
    b.prediction_cost = "inverse_mahalanobis"
    m = matrix()
    evaluate(a, m)
    ra = a.last_result
    ta = [(t.uniqueId, t.cost, t.costMap["prediction"]) for t in a.get_sorted_trajectories()]
    cost_a, flags_a = a._step.engine.costs()
    assert a._step._override is None and a._step.engine.last_predprob_ms == -1.0
    evaluate(b, m)
    tb = [(t.uniqueId, t.cost, t.costMap["prediction"]) for t in b.get_sorted_trajectories()]
    assert ta == tb and ra["best_index"] == b.last_result["best_index"]
    # and the step's own arrays are what they are with the other setting
    c, _ = make_handler()
    c.prediction_cost = "collision_probability"
    evaluate(c, m)
    cost_c, flags_c = c._step.engine.costs()
    assert np.array_equal(cost_a, cost_c) and np.array_equal(flags_a, flags_c)
    assert [t.uniqueId for t in c.get_sorted_trajectories()] != [u for u, _, _ in ta]
    before = c._step
    with pytest.raises(ValueError):
        c.prediction_cost = "other"
        evaluate(c, m)
    assert c._step is before and not before._stale   # (refused before anything was evaluated or replaced)


@pytest.mark.parametrize("wall", ["across", "beside"])
def test_planner_walks_the_restated_order(wall):
    """blocked planner: nothing is collision-free and the planner returns nothing; with a short wall beside the lane (a fifth of
    the selectable candidates collide with it) the first collision-free candidate of the restated order"""
    rp = blocked_planner(engine=None, prediction_cost="collision_probability")
    if wall == "beside":
        w = dict(rp.predictions[5], shape=dict(length=1.0, width=3.0), pos_list=np.tile([[27.0, 2.0]], (31, 1)))
        rp.update_externals(predictions={5: w})
    pair = rp.plan()
    step = rp.last_step
    assert step._override is not None
    v = rp.vehicle_params
    ids, prob, total, flags = _restated(step, rp.predictions, v.length, v.width)
    assert (prob > 0).sum() > len(ids) // 4
    order = ids[np.argsort(total, kind="stable")]
    free = [g for g in order if (flags[g] & _abi.FX_FLAG_SELECTABLE) and not (flags[g] & (_abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY))]
    if wall == "across":
        assert not free and pair is None and rp.optimal_trajectory is None
        return
    assert free and pair is not None and (flags[ids] & _abi.FX_FLAG_COLLISION).any()
    best = rp.optimal_trajectory
    dev = step.engine.prediction_probability(v.length, v.width)
    assert best.uniqueId == dev["best_index"] and best.cost == dev["total"][best.uniqueId]
    key = dict(zip(ids.tolist(), total.tolist()))
    assert best.uniqueId == free[0] or abs(key[best.uniqueId] - key[free[0]]) <= 1e-12 * max(abs(key[free[0]]), 1.0)   # (as above)
    own = int(step.result["best_index"])
    print(f"winner {best.uniqueId} (step's own: {own}), cost {best.cost:.6g}, prediction {best.costMap['prediction']}")


def test_host_boundary_walk_follows_the_override():
    """with a host-side road-boundary check the survivors are walked in the override's order (the top-k holds the step's own):
    a check that rejects the first two candidates it is shown leaves the third collision-free one of the restated order"""
    rp = blocked_planner(engine=None, prediction_cost="collision_probability")
    w = dict(rp.predictions[5], shape=dict(length=1.0, width=3.0), pos_list=np.tile([[27.0, 2.0]], (31, 1)))
    rp.update_externals(predictions={5: w})
    shown = []

    def check(cand):
        shown.append(cand.uniqueId)
        return 1.0 if len(shown) <= 2 else 0
    rp.road_boundary_check = check
    assert rp.plan() is not None
    step = rp.last_step
    v = rp.vehicle_params
    dev = step.engine.prediction_probability(v.length, v.width)
    _, flags = step.engine.costs()
    pool = np.nonzero(((flags & _abi.FX_FLAG_SELECTABLE) != 0) & ((flags & (_abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY)) == 0))[0]
    order = pool[np.argsort(dev["total"][pool], kind="stable")]
    assert shown == order[:3].tolist() and rp.optimal_trajectory.uniqueId == order[2]
    assert rp.optimal_trajectory.boundary_harm == 0 and rp.optimal_trajectory.cost == dev["total"][order[2]]


def test_select_only_configuration_raises():
    rp = blocked_planner(engine=None, prediction_cost="collision_probability", sparse_bundle_k=8)
    with pytest.raises(ValueError, match="bundle"):
        rp.set_cost_function(rp.cost_weights)
    with pytest.raises(ValueError, match="bundle"):
        rp.plan()
    with pytest.raises(ValueError):
        blocked_planner(engine=None, prediction_cost="other").plan()
