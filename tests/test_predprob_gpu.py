"""Collision probability as the prediction cost on the device (fx_predprob_kernel.h) against the NumPy
restatement (tests/predprob_restatement.py) on the device's own read-back planes, and against the reference's own sums
(tests/golden/predprob_*.npz).

Bounds.  Every term of a sum is a probability (at most 1, three rectangles' sum divided by 3), and the suite holds the same
device function, fxrisk::step_probability, to 1e-12 per term (test_risk_gpu.py): a per-obstacle sum of S - 1 terms stays within
(S - 1) 1e-12 absolute, the cost of K such sums within (K (S - 1) + 1) 1e-12.

Re-sum.  The device's cost sum is free of fused multiply-adds (the library is compiled with -ffp-contract=off; finish_candidate
and the obstacle kernel close the sum with a product and an addition per term), and so is NumPy's: the totals are compared
with array_equal, not within ulps."""
import json
import os

import numpy as np
import pytest

from tests import predprob_restatement as pp
from tests.test_risk_gpu import _predictions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EGO_L, EGO_W = 4.508, 1.61
GRID = (8, 16, 16)
COSTED, SELECTABLE = 0x10, 0x20
ALL_COSTS = dict(acceleration=0.3, distance_to_obstacles=0.1, distance_to_reference_path=5.0, jerk=0.15, lane_center_offset=2.0,
                 lateral_jerk=0.2, longitudinal_jerk=0.2, orientation_offset=0.4, path_length=0.05, prediction=0.2, velocity_offset=1.0)
MEASURED = {}


def _make(**kw):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    args = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=GRID, n_obstacles=4)
    args.update(kw)
    return synthetic.make_inputs(**args)


def _engine(inp):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    return FrenetEngine(max_candidates=inp.n_candidates, device=0)


def _tables(preds):
    from frenetix_motion_planner_amd import risk
    return risk.obstacle_tables(preds, {k: "car" for k in preds})


@pytest.fixture(scope="module")
def step():
    inp = _make()
    eng = _engine(inp)
    eng.plan_step(inp)
    cost, flags = eng.costs()
    planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}   # [C, S]
    yield eng, inp, cost, flags, planes
    eng.close()


@pytest.fixture(scope="module")
def full8(step):
    """the K = 8 obstacles, the full call and the restatement on the costed candidates -- computed once, left unchanged"""
    eng, inp, cost, flags, planes = step
    preds, _ = _predictions(planes, flags, np.random.default_rng(7), n_obs=8)
    ids = np.nonzero(flags & COSTED)[0]
    want = pp.prediction_probability(planes["x"][ids], planes["y"][ids], planes["theta"][ids], preds, EGO_L, EGO_W)
    eng.set_risk_obstacles(_tables(preds))
    res = eng.prediction_probability(EGO_L, EGO_W, per_obstacle=True)
    return preds, ids, want, res


def _set8(step, full8):
    step[0].set_risk_obstacles(_tables(full8[0]))


@pytest.mark.parametrize("K", [0, 1, 8, 20])
def test_device_matches_restatement(step, K):
    eng, inp, cost, flags, planes = step
    S = inp.n_samples
    preds, _ = _predictions(planes, flags, np.random.default_rng(7), n_obs=K) if K else ({}, {})
    eng.set_risk_obstacles(_tables(preds))
    res = eng.prediction_probability(EGO_L, EGO_W, per_obstacle=True)
    ids = np.nonzero(flags & COSTED)[0]
    rest = np.setdiff1d(np.arange(inp.n_candidates), ids)
    assert len(ids) > 100 and len(rest) > 0
    assert np.all(np.isnan(res["prob"][rest])) and np.all(np.isnan(res["total"][rest])) and np.all(np.isnan(res["prob_obs"][rest]))
    assert res["prob_obs"].shape == (inp.n_candidates, K)
    prob, prob_obs, steps = pp.prediction_probability(planes["x"][ids], planes["y"][ids], planes["theta"][ids], preds, EGO_L, EGO_W)
    if K == 0:
        assert np.all(res["prob"][ids] == 0.0)
    else:
        rhos = {round(float(p["cov_list"][-1][1, 0] / np.sqrt(p["cov_list"][-1][0, 0] * p["cov_list"][-1][1, 1])), 3) for p in preds.values()}
        assert K < 8 or {0.0, 0.2, -0.6, 0.8, -0.95, 0.99} <= rhos
        assert {len(p["pos_list"]) for p in preds.values()} <= {S - 1, S - 7}
    if K >= 8:
        assert (prob > 0).sum() > len(ids) // 4, "too few candidates near an obstacle"
    e_obs = float(np.abs(res["prob_obs"][ids] - prob_obs).max()) if K else 0.0
    e_sum = float(np.abs(res["prob"][ids] - prob).max())
    print(f"K = {K}: largest error per obstacle {e_obs:.3e} (bound {(S - 1) * 1e-12:.1e}), of the cost {e_sum:.3e} "
          f"(bound {(K * (S - 1) + 1) * 1e-12:.1e}); {int((prob > 0).sum())} of {len(ids)} costed candidates with a positive sum")
    MEASURED[f"K{K}"] = dict(prob_obs_abs_err=e_obs, prob_abs_err=e_sum, costed=int(len(ids)), positive=int((prob > 0).sum()))   # (no times: the file is the same after every run)
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "predprob"), exist_ok=True)
        json.dump(dict(grid=list(GRID), S=S, largest_error=MEASURED), open(os.path.join(ROOT, "profiles", "predprob", "measured.json"), "w"),
                  indent=1, sort_keys=True)
    except OSError:
        pass   # (a read-only checkout: the figures were printed)
    assert e_obs <= (S - 1) * 1e-12
    assert e_sum <= (K * (S - 1) + 1) * 1e-12


def test_id_lists_and_selection(step, full8):
    eng, inp, cost, flags, planes = step
    preds, ids, want, res = full8
    _set8(step, full8)
    sel = np.nonzero(flags & SELECTABLE)[0]
    assert (res["prob"][sel] > 0).sum() >= len(sel) / 4
    rng = np.random.default_rng(1)
    for name, lst in (("100 entries", np.sort(rng.choice(ids, 100, replace=False))),
                      ("unsorted with a duplicate", np.concatenate([rng.permutation(ids)[:77], ids[5:6], ids[5:6]])),
                      ("with candidates that have no cost", np.arange(0, inp.n_candidates, 9))):
        r = eng.prediction_probability(EGO_L, EGO_W, ids=lst, per_obstacle=True)
        costed = (flags[lst] & COSTED) != 0
        for k in ("prob", "total", "prob_obs"):
            assert np.array_equal(r[k][costed], res[k][lst[costed]]), (name, k)
            assert not np.isnan(r[k]).any(), (name, k)   # (a listed candidate is evaluated whatever its flags say)
        assert r["best_index"] == pp.best_index(r["total"], flags[lst], lst), name
    # ids = None: NaN rows, skipped by the arg-min
    assert res["best_index"] == pp.best_index(res["total"], flags)
    assert res["best_index"] >= 0 and res["best_cost"] == res["total"][res["best_index"]]


def test_chunk_size_and_repeatability(step, full8):
    from frenetix_motion_planner_amd._lib import lib
    eng, inp, cost, flags, planes = step
    preds, ids, want, res = full8
    _set8(step, full8)
    S = inp.n_samples
    assert (S - 1) % 7 != 0
    try:
        for cs in (1, 7, S - 1):
            lib().fx_predprob_set_chunk_steps(cs)
            assert lib().fx_predprob_chunk_steps(inp.n_candidates, S, 8) == cs
            r = eng.prediction_probability(EGO_L, EGO_W, per_obstacle=True)
            for k in ("prob", "prob_obs", "total"):
                assert np.array_equal(r[k], res[k], equal_nan=True), (cs, k)
    finally:
        lib().fx_predprob_set_chunk_steps(0)
    a = eng.prediction_probability(EGO_L, EGO_W, per_obstacle=True)
    b = eng.prediction_probability(EGO_L, EGO_W, per_obstacle=True)
    for k in ("prob", "prob_obs", "total"):
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], res[k], equal_nan=True)
    assert a["best_index"] == b["best_index"] == res["best_index"]
    assert eng.last_predprob_ms > 0


@pytest.mark.parametrize("case", ["split", "fused", "eleven_terms"])
def test_step_source_is_the_step_cost(case):
    """source="step": the re-sum with the step's own prediction entry is the step's cost bit for bit -- for a step whose obstacle
    stage ran as its own kernel (the sum closed there), inside the walk, and for the generic kernel with all eleven terms"""
    from frenetix_motion_planner_amd import risk
    kw = dict(cost_weights=dict(ALL_COSTS), lanelets=(3.5, 60)) if case == "eleven_terms" else {}
    inp = _make(**kw)
    with _engine(inp) as eng:
        if case != "eleven_terms":
            eng.set_obstacle_stage(2 if case == "split" else 1)
        eng.plan_step(inp)
        if case == "eleven_terms":
            assert len(inp.cost_names) == 11
        cost, flags = eng.costs()
        eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
        r = eng.prediction_probability(EGO_L, EGO_W, source="step")
        ids = np.nonzero(flags & COSTED)[0]
        assert len(ids) > 100
        assert np.array_equal(r["total"][ids], cost[ids]), case
        n_pred = inp.cost_names.index("prediction")
        raw = eng.costmap()
        assert np.array_equal(r["prob"][ids], raw[ids, n_pred])
        assert (raw[ids, n_pred] > 0).any()
        # K = 0: prob = 0, total = the re-sum without the term
        z = eng.prediction_probability(EGO_L, EGO_W)
        assert np.all(z["prob"][ids] == 0.0)
        assert np.array_equal(z["total"][ids], pp.resum(raw[ids], inp._cost_w, n_pred, 0.0))
        info = eng.step_info()
        print(case, info)
        if case != "eleven_terms":
            assert bool(info["obstacle_kernel"]) == (case == "split")


def test_resum_with_the_probability(step, full8):
    """FMA-free on both sides (module docstring): array_equal.  Behind the prediction the default cost list has one term, so the
    order of a step that deferred its obstacle stage and of one that did not are the same additions."""
    eng, inp, cost, flags, planes = step
    preds, ids, want, res = full8
    n_pred = inp.cost_names.index("prediction")
    assert n_pred + 2 >= len(inp.cost_names)
    raw = eng.costmap()
    assert np.array_equal(res["total"][ids], pp.resum(raw[ids], inp._cost_w, n_pred, res["prob"][ids]))
    assert np.array_equal(eng.costs()[0], cost)   # (the pass wrote nothing the step owns)


def test_empty_pool_and_nan_totals(step, full8):
    eng, inp, cost, flags, planes = step
    _set8(step, full8)
    out = np.nonzero((flags & SELECTABLE) == 0)[0][:50]
    assert len(out) > 0
    r = eng.prediction_probability(EGO_L, EGO_W, ids=out)
    assert r["best_index"] == -1 and np.isnan(r["best_cost"])
    # an infinite weight of the prediction term: the total is NaN (inf x 0) where the probability is zero and +inf elsewhere --
    # selectable candidates with a NaN total, which the arg-min skips
    # -- one obstacle standing at the end point of a late candidate: out of the gate of the candidates that end elsewhere
    S = inp.n_samples
    c0 = np.nonzero(((flags & SELECTABLE) != 0) & ((flags & 0x44) == 0))[0][-1]
    far = {1: dict(pos_list=np.tile([[planes["x"][c0, -1], planes["y"][c0, -1]]], (S - 1, 1)), cov_list=np.tile(np.eye(2) * 0.3, (S - 1, 1, 1)),
                   orientation_list=np.full(S - 1, planes["theta"][c0, -1]), v_list=np.zeros(S - 1), shape=dict(length=4.5, width=1.8))}
    inp2 = _make(cost_weights=dict(inp.cost_weights, prediction=np.inf))
    with _engine(inp2) as e2:
        e2.plan_step(inp2)
        _, f2 = e2.costs()
        e2.set_risk_obstacles(_tables(far))
        r = e2.prediction_probability(EGO_L, EGO_W)
        pool = ((f2 & SELECTABLE) != 0) & ((f2 & 0x44) == 0)
        assert np.isnan(r["total"][pool]).any() and np.isinf(r["total"][pool]).any()
        assert r["best_index"] == pp.best_index(r["total"], f2) and r["best_index"] >= 0
        assert np.isinf(r["best_cost"]) and r["prob"][r["best_index"]] > 0


def test_refusals_leave_the_state_readable():
    from frenetix_motion_planner_amd import risk
    cases = {"no costmap": dict(write_costmap=False), "no bundle and unlisted ids": dict(write_bundle=False),
             "no prediction term": dict(cost_weights=dict(lateral_jerk=0.2, velocity_offset=1.0))}
    for name, kw in cases.items():
        inp = _make(**kw)
        with _engine(inp) as eng:
            eng.plan_step(inp)
            cost, flags = eng.costs()
            eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
            before = eng.device_bytes
            ids = np.nonzero(flags & COSTED)[0][:10]
            with pytest.raises(ValueError):
                eng.prediction_probability(EGO_L, EGO_W)
            with pytest.raises(ValueError):
                eng.prediction_probability(EGO_L, EGO_W, ids=ids)
            assert eng.device_bytes == before, name    # (refused before anything was allocated)
            c2, f2 = eng.costs()
            assert np.array_equal(c2, cost) and np.array_equal(f2, flags), name
            assert eng.last_predprob_ms == -1.0
    inp = _make()
    with _engine(inp) as eng:
        eng.plan_step(inp)
        eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
        for bad in (dict(ids=[inp.n_candidates]), dict(ids=[-1]), dict(ego_length=0.0)):
            kw = dict(ego_length=EGO_L, ego_width=EGO_W)
            kw.update(bad)
            with pytest.raises(ValueError):
                eng.prediction_probability(**kw)
        with pytest.raises(ValueError):
            eng.prediction_probability(EGO_L, EGO_W, source="other")


def test_sparse_set_of_a_select_only_step(step, full8):
    eng, inp, cost, flags, planes = step
    preds, ids, want, res = full8
    sub = ids[::5][:120]
    inp2 = _make(write_bundle=False)
    with _engine(inp2) as e2:
        e2.plan_step(inp2)
        e2.set_risk_obstacles(_tables(preds))
        with pytest.raises(ValueError):
            e2.prediction_probability(EGO_L, EGO_W, ids=sub)
        rows = e2.materialise(sub)
        r = e2.prediction_probability(EGO_L, EGO_W, ids=sub[::-1], per_obstacle=True)
        assert np.array_equal(r["prob"], res["prob"][sub[::-1]]) and np.array_equal(r["prob_obs"], res["prob_obs"][sub[::-1]])
        # the re-sum reads the SET's cost rows, which the list kernel closed (never deferred): bit for bit the host re-sum of those
        # rows with the device's prob, and with source="step" the set's own cost.  Against the bundle-mode step the rows come from
        # another kernel, whose cost sums associate differently: rtol 1e-12, the figure tests/test_materialise_gpu.py holds them to
        n_pred = inp.cost_names.index("prediction")
        assert np.array_equal(r["total"], pp.resum(rows["raw_costs"][::-1], inp._cost_w, n_pred, r["prob"]))
        own = e2.prediction_probability(EGO_L, EGO_W, ids=sub, source="step")
        assert np.array_equal(own["total"], rows["cost"]) and np.array_equal(own["prob"], rows["raw_costs"][:, n_pred])
        assert np.allclose(r["total"], res["total"][sub[::-1]], rtol=1e-12, atol=0)
        assert r["best_index"] == pp.best_index(r["total"], flags[sub[::-1]], sub[::-1])


def test_rewritten_inputs_are_refused():
    """fx_update_state without an evaluation: the planes and the cost map are an older step's -- NOT_READY, the state stays
    readable, and the next evaluation makes the pass answer again"""
    from frenetix_motion_planner_amd import risk
    inp = _make()
    with _engine(inp) as eng:
        eng.plan_step(inp)
        cost, flags = eng.costs()
        eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
        ok = eng.prediction_probability(EGO_L, EGO_W, source="step")
        before = eng.device_bytes
        eng.update_state(eng.make_state_update(v_des=inp.v_des + 1.0))
        for kw in (dict(), dict(ids=np.nonzero(flags & COSTED)[0][:10]), dict(source="step")):
            with pytest.raises(ValueError, match="rewritten"):
                eng.prediction_probability(EGO_L, EGO_W, **kw)
        assert eng.device_bytes == before
        c2, f2 = eng.costs()
        assert np.array_equal(c2, cost) and np.array_equal(f2, flags)
        eng.evaluate()
        eng.finish()
        again = eng.prediction_probability(EGO_L, EGO_W, source="step")
        c3, f3 = eng.costs()
        m = (f3 & COSTED) != 0
        assert m.sum() > 100 and np.array_equal(again["total"][m], c3[m])
        assert not np.array_equal(again["total"], ok["total"], equal_nan=True)   # (another desired velocity: other costs)


def test_device_bytes_without_the_pass():
    """a context that never calls the pass reports the device bytes it always did: nothing of the pass is allocated at creation,
    by a plan step, by the obstacle tables or by risk(); the first call takes its scratch -- [K][S - 1][whole tiles] doubles and
    more -- from the risk passes' block, and only from it: it grows the block of a context that made no risk call, and behind
    risk() over all candidates, whose items keep two partials per obstacle and step where the pass keeps one probability, the
    block, which only grows, already holds it"""
    from frenetix_motion_planner_amd import risk
    from tests.test_risk_gpu import BASE, HARM, EGO
    inp = _make()
    need = 8 * 8 * (inp.n_samples - 1) * (-(-inp.n_candidates // 64) * 64)
    seen = []
    for call in (False, True, None):   # None: the pass is the first call on the block
        with _engine(inp) as eng:
            b0 = eng.device_bytes
            eng.plan_step(inp)
            _, flags = eng.costs()
            planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
            preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=8)
            eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
            b1 = eng.device_bytes
            if call is None:
                eng.prediction_probability(EGO_L, EGO_W)
                assert eng.device_bytes - b1 > need
                continue
            eng.risk(risk.risk_params(BASE, HARM, **EGO))
            b2 = eng.device_bytes
            if call:
                eng.prediction_probability(EGO_L, EGO_W)
                assert eng.device_bytes >= b2 and eng.device_bytes - b1 > need
            seen.append((b0, b1, b2))
    assert seen[0] == seen[1]


@pytest.mark.parametrize("name", ["obs5", "mixed_obs6", "config3_obs20"])
def test_device_matches_reference_golden(name):
    """The stored planner inputs on the device, prob at plane_ids against the reference's own sums at 1e-7 max(|want|, 1).  Left
    out (counted, printed, at most 10 %): candidates whose device planes differ from the stored ones by more than 1e-9, or that
    lie within 1e-6 m of the 5 m gate."""
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from tests.fixtures import load_golden, inputs_from_fixture
    from tests.test_risk_golden import FILES, _load
    g, preds, types, _ = _load("risk_" + name)
    want = np.load(os.path.join(GOLDEN, "predprob_" + name + ".npz"))
    ids = g["plane_ids"]
    assert np.array_equal(ids, want["plane_ids"])
    inp = inputs_from_fixture(load_golden(FILES["risk_" + name]), build_obstacle_hulls)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        dev = np.stack([eng.plane(n)[:, ids].T for n in ("x", "y", "theta", "v")], axis=1)   # [n, 4, S]
        rows = (np.abs(dev - g["planes"]) / (1.0 + np.abs(g["planes"]).max(axis=2, keepdims=True))).max(axis=(1, 2))
        off = rows > 1e-9
        near = pp.near_gate(g["planes"][:, 0], g["planes"][:, 1], preds)
        eng.set_risk_obstacles(_tables(preds))
        r = eng.prediction_probability(*want["ego"], ids=ids, per_obstacle=True)
    keep = ~off & ~near
    print(f"{name}: {int(off.sum())} of {len(ids)} candidates off the reference's planes, {int(near.sum())} near the gate, "
          f"{int((~keep).sum())} left out")
    assert (~keep).sum() <= 0.1 * len(ids)
    S, K = g["planes"].shape[2], len(preds)
    for what, got, ref, terms in (("prob", r["prob"], want["prob"], K * (S - 1) + 1), ("prob_obs", r["prob_obs"], want["prob_obs"], S - 1)):
        err = np.abs(got - ref)[keep] / np.maximum(np.abs(ref)[keep], 1.0)
        # what the tolerance can see: at 1e-7 a value below it passes as zero would.  obs5's sums are all below 3e-10 and only two
        # of mixed_obs6's exceed 1e-7, so that bound constrains the device on config3_obs20 alone; the second bound below -- absolute:
        # the device agrees with the restatement to 1e-12 per term and the restatement with these files to 1e-12 (1 + |want|)
        # (test_predprob_restatement.py) -- sees the small ones too
        seen7 = int((np.abs(ref)[keep] > 1e-7).sum())
        seen12 = int((np.abs(ref)[keep] > terms * 1e-12).sum())
        print(f"  {what}: largest error {err.max():.3e} relative, {np.abs(got - ref)[keep].max():.3e} absolute; {seen7} kept values above 1e-7, "
              f"{seen12} above {terms * 1e-12:.1e}")
        assert err.max() <= 1e-7
        assert np.all(np.abs(got - ref)[keep] <= terms * 1e-12 + 1e-12 * (1 + np.abs(ref)[keep]))   # (device to restatement + restatement to file)
        if name == "config3_obs20":
            assert seen7 >= 82
        if name != "obs5":
            assert seen12 >= 2
