"""Trajectory risk on the device (fx_risk_kernel.h) against the NumPy restatement of calc_risk, on the device's own read-back
planes, for every supported harm / probability variant; the arg-min exactly.  DESIGN.md section 11."""
import numpy as np
import pytest

from tests import risk_restatement as rr
from tests.risk_scenes import BASE, HARM  # noqa: F401  (imported by other modules from here)

pytestmark = pytest.mark.gpu

EGO = dict(ego_length=4.508, ego_width=1.61, ego_mass=1239.0)


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


from tests.risk_scenes import predictions as _predictions  # noqa: E402,F401  (imported by other modules under this name)


VARIANTS = [dict(BASE, ignore_angle=i, sym_angle=s, reduced_angle_areas=r) for i in (False, True) for s in (False, True)
            for r in (False, True) if not (i and (s or r))] + [
    dict(BASE, harm_mode="ref_speed", ignore_angle=True), dict(BASE, fast_prob_mahalanobis=True)]


@pytest.mark.parametrize("modes", VARIANTS, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items() if k in ("harm_mode", "ignore_angle", "sym_angle", "reduced_angle_areas", "fast_prob_mahalanobis")))
def test_device_matches_restatement(step, modes):
    from frenetix_motion_planner_amd import risk
    eng, inp, flags, planes = step
    maha = modes["fast_prob_mahalanobis"]
    if maha:   # a zero covariance is singular: np.linalg.inv raises, as in get_inv_mahalanobis_dist
        with pytest.raises(np.linalg.LinAlgError):
            risk.obstacle_tables(*_predictions(planes, flags, np.random.default_rng(7)), mahalanobis=True)
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), zero_cov=not maha)
    tabs = risk.obstacle_tables(preds, typ, mahalanobis=maha)
    risk.check_obstacle_classes(modes, tabs["classes"])
    eng.set_risk_obstacles(tabs)
    params = risk.risk_params(modes, HARM, **EGO)
    ego, obst, idx = eng.risk(params)
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    assert len(ids) > 100
    assert np.all(np.isnan(ego[np.setdiff1d(np.arange(inp.n_candidates), ids)]))
    we, wo = rr.calc_risk(planes["x"][ids], planes["y"][ids], planes["theta"][ids], planes["v"][ids], preds, typ, modes, HARM, **EGO)
    assert (we > 0).sum() > len(ids) // 4, "too few candidates near an obstacle"
    for got, want in ((ego[ids], we), (obst[ids], wo)):
        err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
        assert err.max() < 1e-12, err.max()
    assert idx == rr.min_risk_index(ego[ids], obst[ids], ids)
    # explicit id list: same values, same arg-min
    sub = ids[::3]
    e2, o2, i2 = eng.risk(params, sub)
    assert np.array_equal(e2, ego[sub]) and np.array_equal(o2, obst[sub])
    assert i2 == rr.min_risk_index(ego[sub], obst[sub], sub)


def test_unprotected_gidas(step):
    from frenetix_motion_planner_amd import risk
    eng, inp, flags, planes = step
    modes = dict(BASE, harm_mode="gidas")
    preds, typ = _predictions(planes, flags, np.random.default_rng(11), n_obs=4, types=["pedestrian", "bicycle", "motorcycle", "unknown"])
    tabs = risk.obstacle_tables(preds, typ)
    risk.check_obstacle_classes(modes, tabs["classes"])
    eng.set_risk_obstacles(tabs)
    ego, obst, idx = eng.risk(risk.risk_params(modes, HARM, **EGO))
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    we, wo = rr.calc_risk(planes["x"][ids], planes["y"][ids], planes["theta"][ids], planes["v"][ids], preds, typ, modes, HARM, **EGO)
    assert np.abs(ego[ids] - we).max() < 1e-12 and np.abs(obst[ids] - wo).max() < 1e-12
    assert idx == rr.min_risk_index(ego[ids], obst[ids], ids)


def test_no_obstacles_is_zero_risk(step):
    from frenetix_motion_planner_amd import risk
    eng, inp, flags, planes = step
    eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
    ego, obst, idx = eng.risk(risk.risk_params(BASE, HARM, **EGO))
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    assert np.all(ego[ids] == 0) and np.all(obst[ids] == 0) and idx == ids[0]


@pytest.mark.parametrize("n", [1, 64, 65, 1024, 1025])
def test_argmin_of_all_equal_is_the_lowest_id(step, n):
    """The tie rule of the one-workgroup arg-min (1024 lanes), across lanes, waves and strides: without obstacles every listed
    candidate has risk 0.0, and of a DESCENDING list the lowest id stands in the last lane that has an entry -- of the only wave,
    the last of a full wave, the first of a second wave, the last lane of the workgroup, the first lane's second entry."""
    from frenetix_motion_planner_amd import risk
    eng, inp, flags, planes = step
    eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
    ids = np.arange(inp.n_candidates - 1, inp.n_candidates - 1 - n, -1)
    assert len(ids) == n and ids[-1] == ids.min() > 0
    ego, obst, idx = eng.risk(risk.risk_params(BASE, HARM, **EGO), ids)
    assert np.all(ego == 0) and np.all(obst == 0) and idx == ids[-1]


def test_risk_needs_the_bundle():
    from frenetix_motion_planner_amd import synthetic, risk
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from frenetix_motion_planner_amd._lib import FxError
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, grid=(3, 5, 5), n_obstacles=2, write_bundle=False)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        eng.set_risk_obstacles(risk.obstacle_tables({}, {}))
        with pytest.raises((FxError, ValueError, RuntimeError)):
            eng.risk(risk.risk_params(BASE, HARM, **EGO))


def test_config3_sized_device_matches_restatement():
    """BASELINE config-3 size: 50 388 candidates (19 x 51 x 52), 20 obstacles along candidates so that many (candidate, obstacle,
    step) triples pass the gate, every rho branch; the multi-workgroup risk pass and the arg-min over all of them."""
    from frenetix_motion_planner_amd import synthetic, risk
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(19, 51, 51), n_obstacles=20)
    assert inp.n_candidates == 50388
    modes = dict(BASE, ignore_angle=True)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        _, flags = eng.costs()
        planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(3), n_obs=20)
        rhos = {round(float(p["cov_list"][-1][1, 0] / np.sqrt(p["cov_list"][-1][0, 0] * p["cov_list"][-1][1, 1])), 3)
                for p in preds.values()}
        assert {0.0, 0.2, -0.6, 0.8, -0.95, 0.99} <= rhos
        tabs = risk.obstacle_tables(preds, typ)
        eng.set_risk_obstacles(tabs)
        ego, obst, idx = eng.risk(risk.risk_params(modes, HARM, **EGO))
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    assert len(ids) > 20000
    we, wo = rr.calc_risk(planes["x"][ids], planes["y"][ids], planes["theta"][ids], planes["v"][ids], preds, typ, modes, HARM, **EGO)
    print(f"config 3: {len(ids)} selected, {np.count_nonzero(we)} with a positive risk")
    assert np.count_nonzero(we) > 1000
    for got, want in ((ego[ids], we), (obst[ids], wo)):
        err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
        assert err.max() < 1e-12, err.max()
    assert idx == rr.min_risk_index(ego[ids], obst[ids], ids)
