"""The responsibility cost as a weighted term of the plan step's cost, beside the step (fx_eval_responsibility_cost_agent, DESIGN.md
section 17): resp against the NumPy restatement of get_responsibility_cost (tests/risk_costs_restatement.py) on the device's own
planes and against the reference's stored values (tests/golden/risk_costs_*.npz), at the tolerances tests/test_risk_costs_gpu.py
holds `responsibility` to; total against NumPy bit for bit.

Re-sum.  The device's cost sum is free of fused multiply-adds (-ffp-contract=off), and so is NumPy's: sum = -0.0, sum += w * c per
name in sorted order with w_resp * resp between `prediction` and `velocity_offset`, total = 0.0 + sum; a step whose obstacle stage
ran as its own kernel added the terms behind the prediction as ONE addend, which the new term joins.  array_equal, not ulps."""
import numpy as np
import pytest

from tests import predprob_restatement as pp
from tests import risk_costs_restatement as rcr
from tests.test_predprob_gpu import ALL_COSTS
from tests.test_risk_costs_gpu import _err, _reach_sets
from tests.test_risk_gpu import BASE, EGO, HARM, _predictions

pytestmark = pytest.mark.gpu

GRID = (8, 16, 16)
COSTED, NEED = 0x10, 0xB
W_RESP = 0.5


def _make(**kw):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    args = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=GRID, n_obstacles=4)
    args.update(kw)
    return synthetic.make_inputs(**args)


def _engine(inp):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    return FrenetEngine(max_candidates=inp.n_candidates, device=0)


def _planes(eng):
    return {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}   # [C, S]


def _resum(raw, weights, names, w_resp, resp, deferred, pred=None):
    """module docstring; raw [n, n_cost], names the step's cost names (sorted), pred: the prediction entry instead of the step's"""
    n_pred = names.index("prediction") if "prediction" in names else -1
    at = next((m for m, nm in enumerate(names) if nm > "responsibility"), len(names))
    defer = deferred and n_pred >= 0
    s, tail = np.full(raw.shape[0], -0.0), np.zeros(raw.shape[0])
    for m in range(len(names) + 1):
        terms = [w_resp * resp] if m == at else []
        if m < len(names):
            terms.append(weights[m] * (pred if (m == n_pred and pred is not None) else raw[:, m]))
        for t in terms:
            if defer and m > n_pred:
                tail = tail + t
            else:
                s = s + t
    if defer:
        s = s + tail
    return 0.0 + s


def _setup(eng, inp, flags, planes, K=8):
    """K obstacles along candidates, reach sets on the first ones, the action-space vector: (preds, typ, keys, sets, resp_vec, x0, th0)"""
    from frenetix_motion_planner_amd import risk
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=K) if K else ({}, {})
    keys = list(preds)
    ok = np.nonzero((flags & NEED) == NEED)[0]
    x0 = np.array([planes["x"][ok[0], 0], planes["y"][ok[0], 0]])
    th0 = float(planes["theta"][ok[0], 0]) + 0.5
    sets = _reach_sets(planes, keys, ok[::3], inp.dt)
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
    eng.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples))
    return preds, typ, keys, sets, risk.action_space_responsibility(preds, x0, th0), x0, th0


def _cost(resp):
    from frenetix_motion_planner_amd import risk
    return risk.risk_cost_params([0, 0, 0, 0, 1], responsibility=resp)


@pytest.fixture(scope="module")
def step():
    inp = _make()
    eng = _engine(inp)
    eng.plan_step(inp)
    cost, flags = eng.costs()
    planes = _planes(eng)
    ctx = _setup(eng, inp, flags, planes)
    yield eng, inp, cost, flags, planes, ctx
    eng.close()


@pytest.mark.parametrize("mode", ["action", "reach"])
def test_resp_matches_restatement(step, mode):
    from frenetix_motion_planner_amd import risk
    eng, inp, cost, flags, planes, (preds, typ, keys, sets, resp_vec, x0, th0) = step
    params = risk.risk_params(BASE, HARM, **EGO)
    C, K = inp.n_candidates, len(preds)
    resp = resp_vec if mode == "action" else "reach_set"
    sel = np.nonzero(flags & COSTED)[0]
    sub = sel[::3]
    assert len(sub) > 64 and len(sub) % 64 != 0 and len(sel) < C and 0 < resp_vec.sum() < K
    full = eng.responsibility_cost(params, _cost(resp), W_RESP)
    part = eng.responsibility_cost(params, _cost(resp), W_RESP, ids=sub)
    assert eng.last_risk_ms > 0
    off = np.setdiff1d(np.arange(C), sel)
    for q in ("resp", "total", "ego_risk", "obst_risk"):
        assert full[q].shape == (C,) and np.all(np.isnan(full[q][off])) and not np.isnan(full[q][sel]).any(), q
        assert np.array_equal(part[q], full[q][sub]), q
    # ego_risk / obst_risk: what risk() returns, bit for bit; resp: what risk_costs() returns in that mode
    e, o, _ = eng.risk(params, sub)
    assert np.array_equal(part["ego_risk"], e) and np.array_equal(part["obst_risk"], o)
    assert np.array_equal(part["resp"], eng.risk_costs(params, _cost(resp), sub)["responsibility"])
    P = [planes[n][sub] for n in ("x", "y", "theta", "v")]
    want = rcr.calc_risk_detail(*P, preds, typ, BASE, HARM, **EGO)
    if mode == "action":
        wr = [rcr.responsibility_action_space(want["obst_risk_max"][c], preds, x0, th0) for c in range(len(sub))]
    else:
        wr = [rcr.responsibility_reach_set(P[0][c], P[1][c], inp.dt, sets, want["obst_risk_max"][c], keys)[0] for c in range(len(sub))]
    wr = np.asarray(wr, np.float64)
    err = _err(part["resp"], wr)
    print(f"{mode}: resp {err:.2e} (bound {(2 * K + 1) * 1e-12:.1e}); {int((wr != 0).sum())} of {len(sub)} candidates with a cost")
    assert (wr != 0).sum() > len(sub) // 8
    assert err < (2 * K + 1) * 1e-12
    # the winner: lexicographic (total, index) over the selectable collision-free candidates
    assert full["best_index"] == pp.best_index(full["total"], flags) and full["best_index"] >= 0
    assert full["best_cost"] == full["total"][full["best_index"]]
    assert part["best_index"] == pp.best_index(part["total"], flags[sub], sub)
    # the term moves the order: the step's own winner has another total now
    assert not np.array_equal(full["total"][sel], cost[sel])


@pytest.mark.parametrize("case", ["fused", "split", "eleven_terms"])
def test_total_is_the_resum(case):
    from frenetix_motion_planner_amd import risk
    kw = dict(cost_weights=dict(ALL_COSTS), lanelets=(3.5, 60)) if case == "eleven_terms" else {}
    inp = _make(**kw)
    params = risk.risk_params(BASE, HARM, **EGO)
    with _engine(inp) as eng:
        if case != "eleven_terms":
            eng.set_obstacle_stage(2 if case == "split" else 1)
        eng.plan_step(inp)
        info = eng.step_info()
        deferred = bool(info["obstacle_kernel"])
        if case != "eleven_terms":
            assert deferred == (case == "split")
        else:
            assert len(inp.cost_names) == 11
        cost, flags = eng.costs()
        planes = _planes(eng)
        raw = eng.costmap()
        sel = np.nonzero(flags & COSTED)[0]
        assert len(sel) > 100
        names, w = list(inp.cost_names), np.asarray(inp._cost_w, np.float64)
        assert "prediction" in names and names[-1] == "velocity_offset"
        # K = 0: resp = 0 and the totals are the step's costs, bit for bit
        eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
        z = eng.responsibility_cost(params, _cost("reach_set"), W_RESP)
        assert np.all(z["resp"][sel] == 0.0) and np.array_equal(z["total"][sel], cost[sel])
        assert np.all(z["ego_risk"][sel] == 0.0) and z["best_index"] == pp.best_index(z["total"], flags)
        preds, typ, keys, sets, resp_vec, x0, th0 = _setup(eng, inp, flags, planes)
        for resp in (resp_vec, "reach_set"):
            r = eng.responsibility_cost(params, _cost(resp), W_RESP)
            assert (r["resp"][sel] != 0).sum() > len(sel) // 8
            assert np.array_equal(r["total"][sel], _resum(raw[sel], w, names, W_RESP, r["resp"][sel], deferred)), case
            assert r["best_index"] == pp.best_index(r["total"], flags)
        # with the collision probability as the prediction entry: first that pass, then the re-sum on the host
        prob = eng.prediction_probability(EGO["ego_length"], EGO["ego_width"])["prob"]
        both = eng.responsibility_cost(params, _cost(resp_vec), W_RESP, prediction="probability")
        assert np.array_equal(both["resp"], eng.responsibility_cost(params, _cost(resp_vec), W_RESP)["resp"], equal_nan=True)
        assert np.array_equal(both["total"][sel], _resum(raw[sel], w, names, W_RESP, both["resp"][sel], deferred, pred=prob[sel])), case
        assert both["best_index"] == pp.best_index(both["total"], flags)
        assert (prob[sel] != raw[sel, names.index("prediction")]).any()
        c2, f2 = eng.costs()
        assert np.array_equal(c2, cost) and np.array_equal(f2, flags)   # (the pass wrote nothing the step owns)


def test_refusals_leave_the_state_readable(step):
    from frenetix_motion_planner_amd import risk
    params = risk.risk_params(BASE, HARM, **EGO)
    cases = {"no costmap": dict(write_costmap=False), "no bundle and unlisted ids": dict(write_bundle=False)}
    for name, kw in cases.items():
        inp = _make(**kw)
        with _engine(inp) as eng:
            eng.plan_step(inp)
            cost, flags = eng.costs()
            eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
            before = eng.device_bytes
            for ids in (None, np.nonzero(flags & COSTED)[0][:10]):
                with pytest.raises(ValueError):
                    eng.responsibility_cost(params, _cost("reach_set"), W_RESP, ids=ids)
            assert eng.device_bytes == before, name    # (refused before anything was allocated)
            c2, f2 = eng.costs()
            assert np.array_equal(c2, cost) and np.array_equal(f2, flags), name
    eng, inp, cost, flags, planes, (preds, typ, keys, sets, resp_vec, x0, th0) = step
    ok = eng.responsibility_cost(params, _cost(resp_vec), W_RESP)
    before = eng.device_bytes
    bad = [dict(weight=0.0), dict(weight=float("nan")), dict(ids=[inp.n_candidates]), dict(ids=[-1]),
           dict(cost_params=risk.risk_cost_params([0, 0, 0, 0, 1])),            # (no responsibility mode)
           dict(cost_params=_cost(resp_vec[:-1]))]                              # (a vector for other obstacles)
    for b in bad:
        kw = dict(params=params, cost_params=_cost(resp_vec), weight=W_RESP)
        kw.update(b)
        with pytest.raises(ValueError):
            eng.responsibility_cost(**kw)
    with pytest.raises(ValueError):
        eng.responsibility_cost(params, _cost(resp_vec), W_RESP, prediction="other")
    # an obstacle the detail pass cannot evaluate (np.max of an empty list upstream)
    short = dict(preds)
    k1 = keys[1]
    short[k1] = dict(preds[k1], pos_list=np.zeros((0, 2)), cov_list=np.zeros((0, 2, 2)), orientation_list=np.zeros(0), v_list=np.zeros(0))
    eng.set_risk_obstacles(risk.obstacle_tables(short, typ))
    with pytest.raises(ValueError):
        eng.responsibility_cost(params, _cost(resp_vec), W_RESP)
    assert eng.device_bytes == before
    c2, f2 = eng.costs()
    assert np.array_equal(c2, cost) and np.array_equal(f2, flags)
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
    eng.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples))
    again = eng.responsibility_cost(params, _cost(resp_vec), W_RESP)
    assert all(np.array_equal(again[q], ok[q], equal_nan=True) for q in ("resp", "total", "ego_risk", "obst_risk"))
    # inputs rewritten since the evaluation: the planes and cost rows are an older step's
    with _engine(inp) as e2:
        e2.plan_step(inp)
        e2.set_risk_obstacles(risk.obstacle_tables({}, {}))
        e2.update_state(e2.make_state_update(v_des=inp.v_des + 1.0))
        with pytest.raises(ValueError, match="rewritten"):
            e2.responsibility_cost(params, _cost("reach_set"), W_RESP)


def test_sparse_set_of_a_select_only_step(step):
    """a step that stored neither bundle nor cost map: the pass answers for listed candidates once they are materialised, from the
    set's rows -- the same planes, so the same resp and risks bit for bit; the re-sum reads the SET's cost rows, which the list
    kernel closed (never deferred), and is the host re-sum of those rows"""
    from frenetix_motion_planner_amd import risk
    eng, inp, cost, flags, planes, (preds, typ, keys, sets, resp_vec, x0, th0) = step
    params = risk.risk_params(BASE, HARM, **EGO)
    sub = np.nonzero(flags & COSTED)[0][::5][:120]
    want = eng.responsibility_cost(params, _cost("reach_set"), W_RESP, ids=sub[::-1])
    inp2 = _make(write_bundle=False)
    with _engine(inp2) as e2:
        e2.plan_step(inp2)
        e2.set_risk_obstacles(risk.obstacle_tables(preds, typ))
        e2.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples))
        with pytest.raises(ValueError):
            e2.responsibility_cost(params, _cost("reach_set"), W_RESP, ids=sub)
        rows = e2.materialise(sub)
        r = e2.responsibility_cost(params, _cost("reach_set"), W_RESP, ids=sub[::-1])
        for q in ("resp", "ego_risk", "obst_risk"):
            assert np.array_equal(r[q], want[q]), q
        assert (r["resp"] != 0).any()
        names, w = list(inp.cost_names), np.asarray(inp._cost_w, np.float64)
        assert np.array_equal(r["total"], _resum(rows["raw_costs"][::-1], w, names, W_RESP, r["resp"], False))
        assert np.allclose(r["total"], want["total"], rtol=1e-12, atol=0)   # (the figure tests/test_materialise_gpu.py holds the rows to)
        assert r["best_index"] == pp.best_index(r["total"], flags[sub[::-1]], sub[::-1])


@pytest.mark.parametrize("name", ["risk_costs_obs5", "risk_costs_mixed_obs6", "risk_costs_config3_obs20"])
def test_resp_matches_reference_golden(name):
    """as tests/test_risk_costs_gpu.py compares `responsibility`: the scenario planned on the device, 1e-7 on the candidates that are
    on the reference's planes and not near a discontinuity -- the same exclusions, counted and printed, at most 10 %"""
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from tests.fixtures import load_golden, inputs_from_fixture
    from tests.test_risk_golden import FILES as SOURCES
    g, src, preds, types, sets, variants = rcr.load_golden(name)
    inp = inputs_from_fixture(load_golden(SOURCES[str(g["source"])]), build_obstacle_hulls)
    ids, keys = g["plane_ids"], list(preds)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        dev = np.stack([eng.plane(n)[:, ids].T for n in ("x", "y", "theta", "v")], axis=1)
        rows = (np.abs(dev - src["planes"]) / (1.0 + np.abs(src["planes"]).max(axis=2, keepdims=True))).max(axis=(1, 2))
        same = rows <= 1e-9
        for vi, v in enumerate(variants):
            tag = f"v{vi}"
            modes = {k: x for k, x in v.items() if k != "obstacles"}
            eng.set_risk_obstacles(risk.obstacle_tables(preds, types, mahalanobis=modes["fast_prob_mahalanobis"]))
            eng.set_reach_sets(risk.reach_set_tables(sets, keys, float(g["dt"]), inp.n_samples))
            params = risk.risk_params(modes, HARM, *src["ego"])
            near = rcr.near_discontinuity(src["planes"], preds, modes, g[tag + "_ego_risk_max"], g[tag + "_obst_risk_max"], *src["ego"])
            use = same & ~near
            print(f"{name} {tag}: {int((~same).sum())} of {len(same)} off the reference's planes, {int(near.sum())} near a discontinuity, "
                  f"{int(use.sum())} compared")
            assert use.mean() >= 0.9
            for mode, resp in (("action", g["resp_vector"]), ("reach", "reach_set")):
                out = eng.responsibility_cost(params, _cost(resp), W_RESP, ids=ids)
                for q, gq in (("resp", "resp_" + mode), ("ego_risk", "ego_risk"), ("obst_risk", "obst_risk")):
                    want = g[f"{tag}_{gq}"]
                    bad = np.nonzero((np.abs(out[q] - want) > 1e-7 * np.maximum(np.abs(want), 1.0)) & use)[0]
                    assert len(bad) == 0, (tag, mode, q, bad)
