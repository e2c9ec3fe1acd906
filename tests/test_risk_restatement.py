"""Trajectory risk without a GPU: the restatement's Genz BVN against Owen's T, the product's parameter block against the
reference's model selection, and the combinations that raise."""
import json
import os

import numpy as np
import pytest

from tests import risk_restatement as rr
from frenetix_motion_planner_amd import risk, _abi

HARM = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "harm_parameters.json")))
BASE = dict(harm_mode="log_reg", ignore_angle=False, sym_angle=True, reduced_angle_areas=True, crash_angle_simplified=True,
            fast_prob_mahalanobis=False)


@pytest.mark.parametrize("r", [0.0, 0.1, -0.29, 0.3, -0.5, 0.74, 0.8, -0.9, 0.93, -0.95, 0.99, -0.999, 0.999999])
def test_genz_bvnu_matches_owens_t(r):
    rng = np.random.default_rng(int(abs(r) * 1e6) + (r < 0))
    h = rng.uniform(-4, 4, 200)
    k = rng.uniform(-4, 4, 200)
    genz = rr.bvnu(h, k, r)
    # P(X > h, Y > k) = P(-X < -h, -Y < -k)
    owen = rr.bvn_lower_owens(-h, -k, r)
    assert np.abs(genz - owen).max() < 1e-13, (r, np.abs(genz - owen).max())


def test_rectangle_probability_shim_is_symmetric_in_order():
    cov = np.array([[0.7, 0.2], [0.2, 0.4]])
    p = rr.rect_probability_owens([-1.0, -0.5], [0.3, 0.8], [0.1, 0.0], cov)
    sx, sy = np.sqrt(0.7), np.sqrt(0.4)
    r = 0.2 / sy / sx
    a1, a2, b1, b2 = (-1.0 - 0.1) / sx, -0.5 / sy, (0.3 - 0.1) / sx, 0.8 / sy
    g = ((rr.bvnu(a1, a2, r) - rr.bvnu(b1, a2, r)) - rr.bvnu(a1, b2, r)) + rr.bvnu(b1, b2, r)
    assert abs(p - float(g)) < 1e-14


def _variants():
    out = []
    for ign in (False, True):
        for sym in (False, True):
            for red in (False, True):
                out.append(dict(BASE, ignore_angle=ign, sym_angle=sym, reduced_angle_areas=red))
    out.append(dict(BASE, harm_mode="ref_speed", ignore_angle=True))
    return out


@pytest.mark.parametrize("modes", _variants(), ids=lambda m: f"{m['harm_mode']}-ign{m['ignore_angle']}-sym{m['sym_angle']}-red{m['reduced_angle_areas']}")
def test_params_reproduce_the_reference_bins(modes):
    """The product's FxRiskParams, evaluated the way the kernel does, gives the restatement's harm for angles over
    [-3 pi, 3 pi] (unwrapped) and every bin edge."""
    p = risk.risk_params(modes, HARM, 4.5, 1.8, 1500.0)
    edges = np.array([15, 45, 75, 105, 135, 165]) / 180 * np.pi
    ang = np.concatenate([np.linspace(-3 * np.pi, 3 * np.pi, 2001), edges, -edges, [3 * (45 / 180 * np.pi), -3 * (45 / 180 * np.pi)]])
    dv = np.linspace(0, 40, len(ang))
    ego_f, _ = rr._models(modes, HARM, True)
    want = ego_f(dv, ang.copy())

    def coef(a):
        if p.n_edges == 0 or -p.edges[0] < a < p.edges[0]:
            return 0.0
        for j in range(1, p.n_edges):
            if p.edges[j - 1] <= a < p.edges[j]:
                return p.coef_pos[j]
            if -p.edges[j - 1] >= a > -p.edges[j]:
                return p.coef_neg[j]
        return p.coef_else
    if p.prot_model == _abi.FX_RISK_HARM_LOGISTIC:
        got = np.array([1 / (1 + np.exp(((-p.prot_c) - p.prot_s * d) - coef(a))) for d, a in zip(dv, ang)])
    else:
        got = np.array([(d / p.prot_ref) ** p.prot_exp if d < p.prot_ref else 1.0 for d in dv])
    assert np.all(np.abs(got - want) <= 1e-14 * np.abs(want))   # (scalar vs vectorised pow may differ in the last bit)


def test_errors():
    with pytest.raises(NotImplementedError):
        risk.risk_params(dict(BASE, crash_angle_simplified=False), HARM, 4.5, 1.8, 1500.0)
    with pytest.raises(ValueError):
        risk.risk_params(dict(BASE, harm_mode="nope"), HARM, 4.5, 1.8, 1500.0)
    with pytest.raises(ValueError):
        risk.check_obstacle_classes(dict(BASE, harm_mode="gidas"), {1: True})
    with pytest.raises(ValueError):
        risk.check_obstacle_classes(BASE, {1: None})
    with pytest.raises(ValueError):
        risk.check_obstacle_classes(dict(BASE, harm_mode="ref_speed"), {1: True})
    risk.check_obstacle_classes(dict(BASE, harm_mode="gidas"), {1: False})
    with pytest.raises(ValueError):
        risk.type_key("spaceship")
    with pytest.raises(ValueError):
        risk.obstacle_tables({1: {}}, {})
    for modes in (dict(BASE, harm_mode="gidas"),):
        with pytest.raises(ValueError):
            rr._models(modes, HARM, True)
    with pytest.raises(ValueError):
        rr._models(BASE, HARM, None)


def test_obstacle_mass():
    assert risk.obstacle_mass("car", 8.1) == -1333.5 + 526.9 * np.power(8.1, 0.8)
    assert risk.obstacle_mass("PRIORITY_VEHICLE", 8.1) == risk.obstacle_mass("car", 8.1)
    assert risk.obstacle_mass("truck", 30.0) == 25000 and risk.obstacle_mass("pedestrian", 0.5) == 75
    assert risk.obstacle_mass("unknown", 1.0) == 0
