"""Per-obstacle risk and harm, risk-cost principles and responsibility on the device (fx_risk_kernel.h)
against the NumPy restatement (tests/risk_costs_restatement.py) on the device's own read-back planes, and against the
reference's own results (tests/golden/risk_costs_*.npz).

Tolerances, on max(|want|, 1), from the 1e-12 the project holds per value: per-obstacle columns 1e-12; a sum of 2K + 1 such
values (2K + 1) 1e-12; maximin 10 x 1e-12 (d(x^10) = 10 x^9 dx, x <= 1); the total the weighted sum of its terms' bounds."""
import json
import os

import numpy as np
import pytest

from tests import risk_costs_restatement as rcr
from tests.test_risk_gpu import BASE, EGO, HARM, _predictions

pytestmark = pytest.mark.gpu

COLS = ("ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max")
WEIGHTS = [1.0, 0.5, 2.0, 0.25, 1.5]
COEFF = (-4.591, 0.185)
CASES = [(0, BASE), (1, BASE), (8, BASE), (8, dict(BASE, ignore_angle=True, sym_angle=False, reduced_angle_areas=False)),
         (8, dict(BASE, harm_mode="ref_speed", ignore_angle=True)), (8, dict(BASE, fast_prob_mahalanobis=True)), (20, BASE)]


@pytest.fixture(scope="module")
def step():
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(8, 16, 16), n_obstacles=4)
    eng = FrenetEngine(max_candidates=inp.n_candidates, device=0)
    eng.plan_step(inp)
    cost, flags = eng.costs()
    planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}   # [C, S]
    yield eng, inp, flags, planes
    eng.close()


from tests.risk_scenes import err as _err, reach_sets as _reach_sets  # noqa: E402,F401


@pytest.mark.parametrize("K,modes", CASES, ids=lambda v: str(v) if isinstance(v, int) else "-".join(
    f"{k}={x}" for k, x in v.items() if k in ("harm_mode", "ignore_angle", "fast_prob_mahalanobis")))
def test_device_matches_restatement(step, K, modes):
    from frenetix_motion_planner_amd import risk
    eng, inp, flags, planes = step
    C = inp.n_candidates
    maha = modes["fast_prob_mahalanobis"]
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=K, zero_cov=not maha) if K else ({}, {})
    tabs = risk.obstacle_tables(preds, typ, mahalanobis=maha)
    risk.check_obstacle_classes(modes, tabs["classes"])
    eng.set_risk_obstacles(tabs)
    params = risk.risk_params(modes, HARM, **EGO)
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    sub = ids[::3]
    assert len(sub) > 64 and len(sub) % 64 != 0 and len(ids) < C
    keys = list(preds)
    x0 = np.array([planes["x"][ids[0], 0], planes["y"][ids[0], 0]])
    th0 = float(planes["theta"][ids[0], 0]) + 0.5
    rng = np.random.default_rng(5)
    bh_all = np.where(rng.random(C) < 0.4, 1.0 / (1.0 + np.exp(-COEFF[0] - COEFF[1] * planes["v"][:, 7])), 0.0)
    resp_vec = risk.action_space_responsibility(preds, x0, th0)
    sets = _reach_sets(planes, keys, sub, inp.dt)
    eng.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples))

    # the restatement, once, on the listed candidates
    P = [planes[n][sub] for n in ("x", "y", "theta", "v")]
    want = rcr.calc_risk_detail(*P, preds, typ, modes, HARM, **EGO)
    if K >= 8:
        assert (want["ego_risk"] > 0).sum() > len(sub) // 4, "too few candidates near an obstacle"
        assert 0 < resp_vec.sum() < K

    e0, o0, i0 = eng.risk(params)
    e1, o1, i1 = eng.risk(params, sub)
    for mode, resp in (("action", resp_vec), ("reach", "reach_set")):
        full = eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, boundary_harm=bh_all, responsibility=resp))
        part = eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, boundary_harm=bh_all[sub], responsibility=resp), sub)
        # bit for bit what risk() returns; NaN rows for the candidates that are not selected; the id list gives the same values
        assert np.array_equal(full["ego_risk"], e0, equal_nan=True) and np.array_equal(full["obst_risk"], o0, equal_nan=True)
        assert np.array_equal(part["ego_risk"], e1) and np.array_equal(part["obst_risk"], o1)
        assert full["min_risk_index"] == i0 and part["min_risk_index"] == i1
        off = np.setdiff1d(np.arange(C), ids)
        for q, a in full.items():
            if isinstance(a, np.ndarray):
                assert a.shape == ((C, K) if q in COLS else (C,)), q
                assert np.all(np.isnan(a[off])) and not np.any(np.isnan(a[ids])), q
                assert np.array_equal(part[q], a[sub]), q
        # per-obstacle columns and calc_risk's scalars
        for q in COLS + ("ego_risk", "obst_risk", "obst_harm_occ"):
            err = _err(part[q], want[q])
            print(f"K={K} {mode} {q}: {err:.2e}")
            assert err < 1e-12, (q, err)
        # principles
        if mode == "action":
            wr = [rcr.responsibility_action_space(want["obst_risk_max"][c], preds, x0, th0) for c in range(len(sub))]
        else:
            rs = [rcr.responsibility_reach_set(P[0][c], P[1][c], inp.dt, sets, want["obst_risk_max"][c], keys) for c in range(len(sub))]
            wr = [r[0] for r in rs]
            if K >= 8:   # both outcomes, on obstacles whose risk is positive: a wrong containment shows in the cost
                hit = np.array([[(np.asarray(h) * (np.array([list(p)[0] for p in sets[k]]) > 0)).any() for h, k in zip(r[1], sets)]
                                for r in rs])
                pos = want["obst_risk_max"][:, :hit.shape[1]] > 0
                assert (hit & pos).any() and (~hit & pos).any()
            # containment exactly: the device's cost is the restated one on the device's own column values, bit for bit
            dev = [rcr.responsibility_reach_set(P[0][c], P[1][c], inp.dt, sets, part["obst_risk_max"][c], keys)[0] for c in range(len(sub))]
            assert np.array_equal(part["responsibility"], np.asarray(dev, np.float64) if K else np.zeros(len(sub)))
        wc = rcr.costs(want, bh_all[sub], WEIGHTS, wr)
        tol = dict(bayes=(2 * K + 1) * 1e-12, equality=(2 * K + 1) * 1e-12, maximin=10e-12, ego=(2 * K + 1) * 1e-12,
                   responsibility=(2 * K + 1) * 1e-12)
        tol["total"] = sum(w * tol[n] for w, n in zip(WEIGHTS, rcr.NAMES))
        for q, t in tol.items():
            err = _err(part[q], wc[q])
            print(f"K={K} {mode} {q}: {err:.2e} (bound {t:.1e})")
            assert err < t, (q, err)
        assert np.array_equal(part["boundary_harm"], bh_all[sub])
        # arg-min of the total: exact
        assert full["min_cost_index"] == rcr.argmin_index(full["total"], np.arange(C))
        assert part["min_cost_index"] == rcr.argmin_index(part["total"], sub)
        assert part["min_cost_index"] == rcr.argmin_index(wc["total"], sub) or np.sort(wc["total"])[1] - np.sort(wc["total"])[0] < 1e-9
    det = eng.risk_detail(params, sub)
    assert "total" not in det and all(np.array_equal(det[q], part[q]) for q in COLS + ("obst_harm_occ",))
    assert eng.last_risk_ms > 0


def test_empty_harm_list_is_refused(step):
    """an obstacle with min(S - 1, len(pos_list)) == 0: np.max of an empty list upstream -> ValueError; risk() keeps skipping it"""
    from frenetix_motion_planner_amd import risk
    eng, inp, flags, planes = step
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=2)
    preds[101] = dict(preds[101], pos_list=np.zeros((0, 2)), cov_list=np.zeros((0, 2, 2)), orientation_list=np.zeros(0), v_list=np.zeros(0))
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
    params = risk.risk_params(BASE, HARM, **EGO)
    eng.risk(params)
    with pytest.raises(ValueError):
        eng.risk_detail(params)
    # a reach-set obstacle index / step outside what the step holds
    eng.set_risk_obstacles(risk.obstacle_tables({100: preds[100]}, typ))
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    t = risk.reach_set_tables({100: [{0.3: sq}]}, [100], inp.dt)
    for bad in (dict(t, entry_obs=np.array([1], np.int32)), dict(t, part_step=np.array([inp.n_samples], np.int32))):
        eng.set_reach_sets(bad)
        with pytest.raises(ValueError):
            eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, responsibility="reach_set"))
    eng.set_reach_sets(t)
    eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, responsibility="reach_set"))


def test_boundary_harm_derived_from_the_step():
    """FX_RISK_BOUNDARY_STEP against TrajectorySample.boundary_harm on a step that ran the road-boundary stage; 0 on one that did not"""
    from frenetix_motion_planner_amd import synthetic, risk, _abi
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from frenetix_motion_planner_amd.trajectories import PlanStepResult
    params = risk.risk_params(dict(BASE, ignore_angle=True), HARM, **EGO)
    for half_width in (1.2, None):
        inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(4, 8, 12), n_obstacles=2,
                                    road_half_width=half_width)
        with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
            res = eng.plan_step(inp)
            assert bool(inp.mode & _abi.FX_MODE_ROAD_BOUNDARY) == (half_width is not None)
            st = PlanStepResult(eng, inp, res, 0)
            _, flags = eng.costs()
            planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
            preds, typ = _predictions(planes, flags, np.random.default_rng(3), n_obs=1)
            eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
            ids = np.nonzero(flags & _abi.FX_FLAG_SELECTABLE)[0] if half_width else np.nonzero((flags & 0xB) == 0xB)[0]
            out = eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, boundary_harm="step", harm_coeff=st.harm_coeff), ids)
            if half_width is None:
                assert not out["boundary_harm"].any()
                continue
            want = np.array([st.sample(int(g)).boundary_harm for g in ids], np.float64)
            assert (want > 0).sum() > 5 and (want == 0).sum() > 5
            assert _err(out["boundary_harm"], want) < 1e-12
            assert _err(out["ego"], out["ego_risk_max"].sum(axis=1) + want) < 3e-12


def _same(got, want):
    if isinstance(want, dict):
        return got.keys() == want.keys() and all(_same(got[k], want[k]) for k in want)
    if isinstance(want, tuple):
        return len(got) == len(want) and all(_same(a, b) for a, b in zip(got, want))
    return np.array_equal(got, want, equal_nan=True) if isinstance(want, np.ndarray) else got == want


def test_calls_share_one_block():
    """risk(), risk_detail() and risk_costs() of an engine share one grow-only device block.  Whatever ran
    before on it, every call returns bit for bit what it returns on a fresh engine that planned the same step and made only that
    call; the block keeps the size of the first, largest call; the engine opened after close() starts from the same device_bytes.
    Grid (6, 7, 3): 168 candidates, 74 of them selected -- the smallest synthetic grid with at least 65 selected candidates
    ((3, 5, 9) has 150 and 32), both counts ragged in their last wave.  Found on the CPU: oracle.plan_step's flags of the grids
    (a, b, c) with a in 2..6, b in 3..9, c in 3..13, in the order of their candidate counts a b (c + 1)."""
    from frenetix_motion_planner_amd import synthetic, risk
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(6, 7, 3), n_obstacles=2)
    params = risk.risk_params(BASE, HARM, **EGO)

    def planned():
        e = FrenetEngine(max_candidates=inp.n_candidates, device=0)
        e.plan_step(inp)
        return e

    eng = planned()
    bytes0 = eng.device_bytes
    _, flags = eng.costs()
    planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    assert inp.n_candidates % 64 != 0 and len(ids) >= 65 and len(ids) % 64 != 0
    preds, typ = _predictions(planes, flags, np.random.default_rng(11), n_obs=3)
    keys = list(preds)
    bh = np.linspace(0.0, 0.9, len(ids))

    def tables(e, K):
        e.set_risk_obstacles(risk.obstacle_tables({k: preds[k] for k in keys[:K]}, typ))
        if K:
            e.set_reach_sets(risk.reach_set_tables(_reach_sets(planes, keys[:K], ids, inp.dt), keys[:K], inp.dt, inp.n_samples))

    def costs(e):
        return e.risk_costs(params, risk.risk_cost_params(WEIGHTS, boundary_harm=bh, responsibility="reach_set"), ids)

    calls = [(3, costs), (3, lambda e: e.risk(params, ids[::3])), (0, lambda e: e.risk_detail(params)), (0, lambda e: e.risk(params, ids)),
             (1, costs), (3, costs)]
    want = []
    for j, (K, call) in enumerate(calls):
        if j == 5:   # (the first call again)
            want.append(want[0])
            continue
        with planned() as e:
            assert e.device_bytes == bytes0
            tables(e, K)
            want.append(call(e))
    assert np.nanmax(want[0]["obst_risk_max"]) > 0   # (not a comparison of zeros)

    sizes, last = [], None
    for (K, call), w in zip(calls, want):
        if K != last:
            tables(eng, K)
        last = K
        assert _same(call(eng), w), len(sizes)
        sizes.append(eng.device_bytes)
    assert sizes[0] > bytes0 and sizes == [sizes[0]] * len(calls)
    eng.close()
    with planned() as e:
        assert e.device_bytes == bytes0


@pytest.mark.parametrize("name", ["risk_costs_obs5", "risk_costs_mixed_obs6", "risk_costs_config3_obs20"])
def test_device_matches_reference_golden(name):
    """as test_risk_golden.test_device_matches_reference_golden: the scenario planned on the device, 1e-7 on the candidates that
    are on the reference's planes and not near a discontinuity; at most 10 % left out"""
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
            tabs = risk.obstacle_tables(preds, types, mahalanobis=modes["fast_prob_mahalanobis"])
            eng.set_risk_obstacles(tabs)
            eng.set_reach_sets(risk.reach_set_tables(sets, keys, float(g["dt"]), inp.n_samples))
            params = risk.risk_params(modes, HARM, *src["ego"])
            near = rcr.near_discontinuity(src["planes"], preds, modes, g[tag + "_ego_risk_max"], g[tag + "_obst_risk_max"], *src["ego"])
            use = same & ~near
            print(f"{name} {tag}: {int((~same).sum())} of {len(same)} off the reference's planes, {int(near.sum())} near a discontinuity, "
                  f"{int(use.sum())} compared")
            assert use.mean() >= 0.9
            for mode, resp in (("action", g["resp_vector"]), ("reach", "reach_set")):
                out = eng.risk_costs(params, risk.risk_cost_params(g["weights"], boundary_harm=g["boundary_harm"], responsibility=resp), ids)
                names = {q: q for q in COLS + ("ego_risk", "obst_risk", "obst_harm_occ", "bayes", "equality", "maximin", "ego")}
                names["responsibility"], names["total"] = "resp_" + mode, "total_" + mode
                for q, gq in names.items():
                    want = g[f"{tag}_{gq}"]
                    bad = np.nonzero((np.abs(out[q] - want) > 1e-7 * np.maximum(np.abs(want), 1.0)).reshape(len(ids), -1).any(axis=1) & use)[0]
                    assert len(bad) == 0, (tag, mode, q, bad)
                s = np.sort(g[f"{tag}_total_{mode}"])
                if use.all() and s[1] - s[0] > 1e-6 * max(abs(s[0]), 1e-300):
                    assert out["min_cost_index"] == int(g[f"{tag}_min_index_{mode}"])
