"""The re-score over effective cost lists and for a whole agent batch (csrc/fx_rescore_batch_kernel.h): what
the tests of that pass share beside tests/rescore_planes.py -- the effective list of a step's cost list in plain Python, the NumPy
reference over it, external rows for the planes of rescore_planes.py, and the per-agent loop a batch call is held to.  Importable
without a GPU."""
import numpy as np

from frenetix_motion_planner_amd import _abi
from tests import device_planes as dp
from tests import rescore_planes as rp

PRED = _abi.COST_ID["prediction"]


def resp_at(cost_ids) -> int:
    """position of the responsibility term in a list of ascending cost ids: in front of the first id above the prediction's, else
    at the end (fx_resp_term_at, csrc/fx_rescore_batch_plan.h)"""
    return next((m for m, i in enumerate(cost_ids) if i > PRED), len(cost_ids))


def effective_rows(raw, cost_ids, pred=None, resp=None):
    """(rows [n_eff][n], n_pred) of the effective list: raw [n_cost][n] with pred in place of the prediction's row and resp
    inserted at resp_at"""
    cost_ids = list(cost_ids)
    n_pred = cost_ids.index(PRED) if PRED in cost_ids else -1
    rows = [np.asarray(r, np.float64) for r in raw]
    if pred is not None:
        assert n_pred >= 0
        rows[n_pred] = np.asarray(pred, np.float64)
    if resp is not None:
        rows.insert(resp_at(cost_ids), np.asarray(resp, np.float64))
    return np.stack(rows) if rows else np.zeros((0, np.shape(raw)[1])), n_pred


def expected(raw, flags, W, cost_ids, deferred, pred=None, resp=None):
    """(winner [W], cost [W], totals [W][n]) over the effective list: rescore_planes.expected -- fx_cost_sum.h operation by
    operation -- with n_cost := n_eff"""
    rows, n_pred = effective_rows(raw, cost_ids, pred, resp)
    assert np.shape(W)[1] == len(rows)
    return rp.expected(rows, flags, W, n_pred, deferred)


_SCENES = {}
SCENES = ("plain", "deferred", "pred_last")


def scene(n: int, kind: str = "plain"):
    """PlanInputs of exactly n candidates that store bundle and cost map (rescore_planes.count_scene, which is "plain"):
    "deferred" has four obstacles, so that an engine told to run the obstacle stage as its own kernel closes the sum there (the
    deferred form); "pred_last" lacks `velocity_offset`: the prediction is the list's last entry and the responsibility term
    lands at the end"""
    import copy

    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
    if kind == "plain":
        return rp.count_scene(n)
    if kind not in _SCENES:
        kw = dict(ref_kind="arc", v0=10.0, grid=(5, 30, 30), horizon=1.5, n_pred=15, as_matrix=True)
        if kind == "deferred":
            _SCENES[kind] = synthetic.make_inputs(hull_builder=build_obstacle_hulls, n_obstacles=4, cost_weights=dict(DEFAULT_COST_WEIGHTS), **kw)
        elif kind == "pred_last":
            w = {k: v for k, v in DEFAULT_COST_WEIGHTS.items() if k != "velocity_offset"}
            _SCENES[kind] = synthetic.make_inputs(n_obstacles=0, cost_weights=w, **kw)
        else:
            raise KeyError(kind)
    inp = copy.copy(_SCENES[kind])
    inp.sampling_matrix = np.ascontiguousarray(inp.sampling_matrix[:n])
    assert inp.n_candidates == n and inp.write_bundle and (inp.mode & _abi.FX_MODE_WRITE_COSTMAP) and "prediction" in inp.cost_names
    return inp


EXTERNAL = ("plain", "non_finite", "breaks_ties")


def external_row(kind: str, n: int, seed: int):
    """a row [n] from outside the step: "plain" values in [0, 1); "non_finite" with NaN, +inf and -inf scattered over it;
    "breaks_ties" multiples of 1/8 that ascend with the index -- on a plane whose own rows are equal for every candidate the row
    alone decides, the lowest index under a positive weight and the highest under a negative one"""
    rng = np.random.default_rng([20251022, seed, n])
    if kind == "plain":
        return rng.uniform(0.0, 1.0, size=n)
    if kind == "non_finite":
        row = rng.uniform(0.0, 1.0, size=n)
        at = rng.random(n) < 0.3
        row[at] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=int(at.sum()))
        return row
    if kind == "breaks_ties":
        return np.arange(n, dtype=np.float64) / 8.0
    raise KeyError(kind)


def same_result(got, winner, cost, what=""):
    """winner equal, cost bit for bit (a winner's cost is never NaN)"""
    assert np.array_equal(got["winner"], winner), (what, got["winner"], winner)
    assert np.array_equal(dp.bits(got["cost"]), dp.bits(cost)), (what, got["cost"], cost)


def loop_of(eng, weights, agents, pred=None, resp=None):
    """the per-agent loop a rescore_batch call replaces, on the same context"""
    pred = [None] * len(agents) if pred is None else pred
    resp = [None] * len(agents) if resp is None else resp
    return [eng.rescore(w, agent=a, pred=p, resp=r) for w, a, p, r in zip(weights, agents, pred, resp)]


def same_as_loop(eng, weights, agents, pred=None, resp=None, what=""):
    got = eng.rescore_batch(weights, agents=agents, pred=pred, resp=resp)
    want = loop_of(eng, weights, agents, pred, resp)
    assert len(got) == len(want) == len(agents)
    for g, w_, a in zip(got, want, agents):
        same_result(g, w_["winner"], w_["cost"], (what, a))
    return got
