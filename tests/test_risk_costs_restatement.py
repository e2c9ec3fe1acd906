"""Risk-cost principles and responsibility, CPU: the NumPy restatement (tests/risk_costs_restatement.py)
against the reference's own calc_risk / get_*_costs / get_responsibility_cost (tests/golden/gen_risk_costs_golden.py) to
1e-12 (1 + |want|) with the arg-min exact; the quirks the device transcribes; the host tables of the product's risk.py."""
import json
import os

import numpy as np
import pytest

from tests import risk_costs_restatement as rcr

HARM = json.load(open(os.path.join(rcr.GOLDEN, "harm_parameters.json")))
FILES = ("risk_costs_obs5", "risk_costs_mixed_obs6", "risk_costs_config3_obs20")   # tests/golden/*.npz
assert FILES == rcr.FILES
CASES = [(name, vi) for name in FILES for vi in range(3)]


def _close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= 1e-12 * (1 + np.abs(want))))


@pytest.mark.parametrize("name,vi", CASES)
def test_restatement_matches_reference_golden(name, vi):
    g, src, preds, types, sets, variants = rcr.load_golden(name)
    modes = {k: x for k, x in variants[vi].items() if k != "obstacles"}
    tag = f"v{vi}"
    P, ids, keys = src["planes"], g["plane_ids"], list(preds)
    assert np.array_equal(ids, src["plane_ids"])
    d = rcr.calc_risk_detail(P[:, 0], P[:, 1], P[:, 2], P[:, 3], preds, types, modes, HARM, *src["ego"])
    for q in ("ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max", "ego_risk", "obst_risk", "obst_harm_occ"):
        assert _close(d[q], g[f"{tag}_{q}"]), q
    pos, th0, dt = g["ego_position"], float(g["ego_orientation"]), float(g["dt"])
    resp_a = [rcr.responsibility_action_space(d["obst_risk_max"][c], preds, pos, th0) for c in range(len(ids))]
    rs = [rcr.responsibility_reach_set(P[c, 0], P[c, 1], dt, sets, d["obst_risk_max"][c], keys) for c in range(len(ids))]
    assert _close(resp_a, g[tag + "_resp_action"]) and _close([r[0] for r in rs], g[tag + "_resp_reach"])
    assert np.array_equal(np.array([np.concatenate(r[1]) for r in rs]), g[tag + "_contain"])   # containment: exact
    for mode, resp in (("action", resp_a), ("reach", [r[0] for r in rs])):
        c = rcr.costs(d, g["boundary_harm"], g["weights"], resp)
        for q in ("bayes", "equality", "maximin", "ego"):
            assert _close(c[q], g[f"{tag}_{q}"]), q
        assert _close(c["total"], g[f"{tag}_total_{mode}"])
        assert rcr.argmin_index(c["total"], ids) == int(g[f"{tag}_min_index_{mode}"])


def test_goldens_cover_the_cases():
    occ = 0
    for name in rcr.FILES:
        g, src, preds, types, sets, variants = rcr.load_golden(name)
        assert [v["fast_prob_mahalanobis"] for v in variants] == [False, False, True] and variants[1]["ignore_angle"]
        bh = g["boundary_harm"]
        assert (bh == 0).any() and ((bh > 0) & (bh < 1)).any()
        assert 0.3 in g["rs_time_t"] and (g["rs_time_t"] == 0).sum() == 1 and len(set(g["rs_vert_count"])) > 2
        assert 0 < g["resp_vector"].sum() < len(preds)
        assert np.count_nonzero(g["v0_ego_risk_max"]) > 0 and np.all(g["v0_ego_harm_max"] > 0)
        occ += np.count_nonzero(g["v0_obst_harm_occ"])
    assert occ > 30   # (a probability above 0.001 is rare on the first two scenarios' trajectories)


def test_no_obstacles_gives_zeros():
    x = np.zeros((3, 5))
    d = rcr.calc_risk_detail(x, x, x, x, {}, {}, dict(harm_mode="log_reg"), HARM, 4.5, 1.6, 1200.0)
    assert d["ego_risk_max"].shape == (3, 0) and not d["ego_risk"].any() and not d["obst_harm_occ"].any()
    c = rcr.costs(d, np.array([0.2, 0.0, 0.7]), [1, 1, 1, 1, 1], resp=None)
    for q in rcr.NAMES + ("total",):
        assert np.array_equal(c[q], np.zeros(3)), q


def test_maximin_gate_keeps_the_harm_where_the_risk_is_below_eps():
    # upstream's comment says "set maximin to 0 if the risk is 0"; the code does the opposite, and is what is transcribed
    assert rcr.maximin([0.0], [0.5], [0.9], [0.8], 0.0) == 0.9 ** 10        # ego risk 0: ego harm kept; obstacle risk 0.5: dropped
    assert rcr.maximin([0.5], [0.5], [0.9], [0.8], 0.3) == 0.3 ** 10        # both risks above eps: only the boundary harm is left
    assert rcr.maximin([0.5], [9.9e-10], [0.9], [0.8], 0.0) == 0.8 ** 10    # below eps = 10e-10
    assert rcr.maximin([0.5], [1.0e-9], [0.9], [0.8], 0.0) == 0.0           # eps itself is not below eps


def test_step_index_truncation():
    from frenetix_motion_planner_amd import risk
    assert list(rcr.time_steps([0.3, 0.5, 1.0, 0.0], 0.1)) == [1, 4, 9, -1]    # 0.3 / 0.1 - 1 = 1.9999999999999996 -> 1
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    t = risk.reach_set_tables({7: [{0.0: sq}, {0.3: sq}, {0.5: sq[:3]}]}, [5, 7], 0.1, n_steps=31)
    assert list(t["part_step"]) == [1, 4] and list(t["part_obs"]) == [1, 1] and list(t["entry_obs"]) == [1]
    assert list(t["entry_part_off"]) == [0, 2] and list(t["part_vert_off"]) == [0, 4, 7] and t["verts"].shape == (7, 2)


def test_refused_inputs_raise_value_error():
    from frenetix_motion_planner_amd import risk
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    with pytest.raises(ValueError):
        risk.reach_set_tables({9: [{0.3: sq}]}, [5, 7], 0.1)                 # not in the predictions (KeyError upstream)
    with pytest.raises(ValueError):
        risk.reach_set_tables({7: [{3.2: sq}]}, [5, 7], 0.1, n_steps=31)     # step 31 of 31 points (IndexError upstream)
    with pytest.raises(ValueError):
        risk.reach_set_tables({7: [{0.3: sq[:2]}]}, [5, 7], 0.1)
    with pytest.raises(ValueError):
        rcr.responsibility_reach_set(np.zeros(31), np.zeros(31), 0.1, {9: [{0.3: sq}]}, [0.0, 0.0], [5, 7])
    with pytest.raises(ValueError):
        rcr.responsibility_reach_set(np.zeros(31), np.zeros(31), 0.1, {7: [{3.2: sq}]}, [0.0, 0.0], [5, 7])
    with pytest.raises(ValueError):
        risk.risk_cost_params([1, 2, 3])
    with pytest.raises(ValueError):
        risk.risk_cost_params(dict(bayes=1, utilitarian=2))
    x = np.zeros((2, 5))
    empty = {3: dict(pos_list=np.zeros((0, 2)), cov_list=np.zeros((0, 2, 2)), orientation_list=np.zeros(0), v_list=np.zeros(0),
                     shape=dict(length=4.0, width=2.0))}
    with pytest.raises(ValueError):
        rcr.calc_risk_detail(x, x, x, x, empty, {3: "car"}, dict(harm_mode="log_reg", ignore_angle=True), HARM, 4.5, 1.6, 1200.0)


def test_host_tables_match_the_golden():
    """risk.action_space_responsibility / risk.reach_set_tables (the product's host side) on the golden's ego state and reach sets"""
    from frenetix_motion_planner_amd import risk
    for name in rcr.FILES:
        g, src, preds, types, sets, _ = rcr.load_golden(name)
        assert np.array_equal(risk.action_space_responsibility(preds, g["ego_position"], float(g["ego_orientation"])), g["resp_vector"])
        t = risk.reach_set_tables(sets, list(preds), float(g["dt"]), n_steps=src["planes"].shape[2])
        live = g["rs_time_t"] > 0
        assert np.array_equal(t["part_step"], rcr.time_steps(g["rs_time_t"][live], float(g["dt"])))
        assert np.array_equal(np.diff(t["part_vert_off"]), g["rs_vert_count"][live]) and len(t["entry_obs"]) == len(sets)
        # containment by the tables, as the kernel walks them, against the reference's cache
        P = src["planes"]
        col = np.nonzero(live)[0]
        for c in range(0, len(P), 7):
            for p in range(len(t["part_step"])):
                poly = t["verts"][t["part_vert_off"][p]:t["part_vert_off"][p + 1]]
                st = t["part_step"][p]
                assert rcr.contains(poly, P[c, 0, st], P[c, 1, st]) == bool(g["v0_contain"][c, col[p]])
