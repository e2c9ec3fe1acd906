"""Scenes, hypotheses and references of the hypotheses pass's GPU tests (FrenetEngine.hypotheses, fx_eval_hypotheses_agent; DESIGN.md
section 25).

A scene is a synthetic plan step of N = 31 steps (S = 32 samples: the 31 steps are divisible by none of 2, 3, 5, so the last chunk
of every steps-per-item choice is short) with K obstacles.  A hypothesis is built at the level a caller has: the predictions dict is
changed, packed with the planner's packer and brought to the upload's K and P by `problem.hypothesis_arrays` -- or, where the case is a
property of the packed arrays themselves (a covariance inverse without a Cholesky factor, a hull that covers everything), the packed
arrays are changed.  The reference of every hypothesis is a REAL step: `update_state` with those arrays and an evaluation on a
second engine under the same forcing (`real_step`), compared exactly (`same_as_real_step`).  Importable without a GPU."""
import copy

import numpy as np

from frenetix_motion_planner_amd import _abi, synthetic
from frenetix_motion_planner_amd.problem import hypothesis_arrays, pack_predictions
from tests import device_planes as dp

COSTED, SEL, COL, BND = _abi.FX_FLAG_COSTED, _abi.FX_FLAG_SELECTABLE, _abi.FX_FLAG_COLLISION, _abi.FX_FLAG_BOUNDARY
HORIZON, N = 3.1, 31
GRIDS = {"small": (3, 5, 7), "mid": (5, 10, 12), "large": (8, 16, 16)}   # 120, 650 and 2 176 candidates
MAX_CANDIDATES = 8 * 16 * 17
KS = (1, 2, 3, 4, 7, 20, 64)
SPIS = (2, 3, 5)


def hull_builder():
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return build_obstacle_hulls


def make(grid, n_obstacles, **kw):
    args = dict(hull_builder=hull_builder(), ref_kind="arc", v0=10.0, grid=grid, n_obstacles=n_obstacles, horizon=HORIZON, n_pred=N,
                lead_gap=25.0)
    args.update(kw)
    inp = synthetic.make_inputs(**args)
    assert inp.N == N and inp.n_samples == N + 1
    if n_obstacles > 20:
        # 64 cars in the generator's 120 m x 12 m corridor leave no collision-free candidate: all but the first eight drive 40 m
        # beside the road -- they still take part in every step's prediction sum and in every cull
        for k in list(inp.predictions)[8:]:
            inp.predictions[k]["pos_list"] = inp.predictions[k]["pos_list"] + np.array([0.0, 40.0])
        inp.obstacles = pack(inp.predictions)
    return inp


def engine(max_candidates=MAX_CANDIDATES, max_obstacles=64, **kw):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    return FrenetEngine(max_candidates=max_candidates, max_steps=N, max_obstacles=max_obstacles, device=0, **kw)


def pack(preds):
    return pack_predictions(preds, N + 1, hull_builder())


def hypotheses_of(inp, winner_xy_theta):
    """name -> hypothesis arrays (K and P of inp's upload) of the cases of the issue.  winner_xy_theta: (x [S], y [S], theta [S]) of the
    base step's winner, the path an obstacle is moved onto."""
    K, P = int(inp.obstacles["K"]), int(inp.obstacles["P"])
    preds = inp.predictions
    keys = list(preds)
    a, b = keys[0], keys[min(1, K - 1)]
    out = {"own": hypothesis_arrays(inp.obstacles, K, P)}
    # obstacle 0 drives along the winner's path: prediction i - 1 meets ego step i
    x, y, th = winner_xy_theta
    moved = copy.deepcopy(preds)
    moved[a] = dict(moved[a], pos_list=np.stack([x[1:], y[1:]], axis=1), orientation_list=np.array(th[1:]))
    out["on_the_winners_path"] = hypothesis_arrays(pack(moved), K, P)
    short = copy.deepcopy(preds)
    short[b] = {k: (v[:10] if k.endswith("_list") else v) for k, v in short[b].items()}
    out["shorter_than_the_horizon"] = hypothesis_arrays(pack(short), K, P)
    assert out["shorter_than_the_horizon"]["npred"][min(1, K - 1)] == 10 < N
    two = copy.deepcopy(preds)
    two[a] = {k: (v[:1] if k.endswith("_list") else v) for k, v in two[a].items()}
    if K > 1:
        two[b] = {k: (v[:2] if k.endswith("_list") else v) for k, v in two[b].items()}
    out["at_most_two_steps"] = hypothesis_arrays(pack(two), K, P)
    assert out["at_most_two_steps"]["npred"][0] == 1 and out["at_most_two_steps"]["nhull"][0] == 0
    nofac = copy.deepcopy(out["own"])
    nofac["cov_inv"][0, :, :] = (1.0, 0.0, 0.0, -1.0)          # indefinite: no Cholesky factor, the kernel's raw-record fall-back
    out["no_cholesky_factor"] = nofac
    out["all_absent"] = hypothesis_arrays(pack({}), K, P)
    assert not out["all_absent"]["npred"].any() and not out["all_absent"]["nhull"].any()
    cover = copy.deepcopy(out["own"])
    cover["hull"][0, :, :] = (float(x[0]), float(y[0]), 1.0, 0.0, 1.0e3, 1.0e3)   # a box of 2 km around the ego's start, every step
    cover["nhull"][0] = P - 1
    out["covers_the_grid"] = cover
    return out


def real_step(e2, hyp, agent=0):
    """the step of e2's resident upload run with the hypothesis' arrays: dict(result, cost, flags, pred column)"""
    e2.update_state(e2.make_state_update(obstacles=hyp), agent)
    e2.evaluate()
    res = e2.finish()[agent]
    cost, flags = e2.costs(agent)
    inp = e2._inputs[agent]
    cm = e2.costmap(agent)
    pred = cm[:, inp.cost_names.index("prediction")] if "prediction" in inp.cost_names else None
    return dict(res=res, cost=cost, flags=flags, pred=pred, shard_begin=inp.shard_begin)


def same_as_real_step(r, h, real, where=""):
    """hypothesis h of the call's answer r against a real step: winner, cost bits, n_collisions, and pred / total / collision of every
    costed candidate, all exact"""
    flags, cost = real["flags"], real["cost"]
    costed = (flags & COSTED) != 0
    assert costed.any(), where
    res = real["res"]
    assert np.array_equal(dp.bits(r["totals"][h][costed]), dp.bits(cost[costed])), where
    assert np.all(np.isnan(r["totals"][h][~costed])), where
    assert np.array_equal(r["collisions"][h][costed], (flags[costed] & COL) != 0), where
    if real["pred"] is not None:
        assert np.array_equal(dp.bits(r["pred"][h][costed]), dp.bits(real["pred"][costed])), where
    if res["best_index"] >= 0:
        assert r["winner"][h] == res["best_index"] - real["shard_begin"], where
        assert dp.bits(r["cost"][h]) == dp.bits(res["best_cost"]), where
    else:
        assert r["winner"][h] == -1 and r["cost"][h] == np.inf, where
    assert r["n_collisions"][h] == res["n_collisions"], where


def numpy_selection(total, col, flags):
    """(winner, cost, n_collisions) of the rule, from a call's own returned rows: the lexicographic (total, index) minimum over
    the selectable candidates without a collision and off no boundary, NaN skipped; the selectable colliding candidates ordered
    before it -- all of them where nothing is eligible"""
    sel = (flags & SEL) != 0
    el = np.nonzero(sel & ~col & ((flags & BND) == 0) & ~np.isnan(total))[0]
    hit = np.nonzero(sel & col)[0]
    if len(el) == 0:
        return -1, np.inf, len(hit)
    g = int(el[np.lexsort((el, total[el]))][0])
    with np.errstate(invalid="ignore"):
        before = (total[hit] < total[g]) | ((total[hit] == total[g]) & (hit < g))
    return g, float(total[g]), int(before.sum())
