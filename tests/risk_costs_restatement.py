"""NumPy restatement of what the reference builds on calc_risk's per-obstacle results (risk_costs.py:84-251,
utility/responsibility.py) -- test infrastructure, written from the reference's Python, independently of the product.

Per-obstacle risk maxima are tests/risk_restatement.calc_risk called with one obstacle at a time; the harm maxima and
obst_harm_occ are rebuilt from its model helpers; the principles and both responsibility modes are literal transcriptions.
Planes x, y, theta, v are [C, L]; per-obstacle results are [C, K] in the order of the predictions' keys.
"""
import json
import os

import numpy as np

from tests import risk_restatement as rr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("risk_costs_obs5", "risk_costs_mixed_obs6", "risk_costs_config3_obs20")

NAMES = ("bayes", "equality", "maximin", "ego", "responsibility")


def _harm(x, y, th, v, pr, key, modes, coeff, ego_mass):
    """(ego_harm, obst_harm) [C, pl] of get_harm (harm_estimation.py:282-300, crash_angle_simplified)"""
    L = x.shape[1]
    ego_f, obs_f = rr._models(modes, coeff, rr.PROTECTION[key])
    pos = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
    yaw = np.asarray(pr["orientation_list"], np.float64)
    vo = np.asarray(pr["v_list"], np.float64)
    pl = min(L - 1, len(pos))
    mass_o = rr._mass(key, pr["shape"]["length"] * pr["shape"]["width"])
    pdof = yaw[:pl] - th[:, :pl] + np.pi
    rel = np.arctan2(pos[:pl, 1] - y[:, :pl], pos[:pl, 0] - x[:, :pl])
    dv = np.sqrt(v[:, :pl] ** 2 + vo[:pl] ** 2 + 2 * v[:, :pl] * vo[:pl] * np.cos(pdof))
    he = np.broadcast_to(ego_f(mass_o / (ego_mass + mass_o) * dv, (rel - th[:, :pl]).copy()), dv.shape)
    ho = np.broadcast_to(obs_f(ego_mass / (ego_mass + mass_o) * dv, (np.pi + rel - yaw[:pl]).copy()), dv.shape)
    return he, ho


def probability(x, y, th, pr, modes, ego_length, ego_width):
    """collision probability list [C, L - 1] of one obstacle (collision_probability.py get_collision_probability_fast /
    get_inv_mahalanobis_dist): entry i - 1 belongs to ego point i, 0 behind the prediction and outside the 5 m gate"""
    C, L = x.shape
    pos = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
    covs = np.asarray(pr["cov_list"], np.float64).reshape(-1, 2, 2)
    yaw = np.asarray(pr["orientation_list"], np.float64)
    length = pr["shape"]["length"]
    off = np.array([ego_length / 6, ego_width / 2])
    prob = np.zeros((C, L - 1))
    inv = np.linalg.inv(covs) if modes.get("fast_prob_mahalanobis") else None
    for i in range(1, min(L, len(pos))):
        m0 = pos[i - 1]
        if inv is not None:
            d0, d1 = x[:, i] - m0[0], y[:, i] - m0[1]
            iv = inv[i - 1]
            r0, r1 = d0 * iv[0, 0] + d1 * iv[1, 0], d0 * iv[0, 1] + d1 * iv[1, 1]
            prob[:, i - 1] = 1.0 / ((r0 * d0 + r1 * d1) ** 2)
            continue
        dev = np.array([np.cos(yaw[i]), np.sin(yaw[i])]) * length / 2
        means = [m0, m0 + dev, m0 - dev]
        dist = np.min([np.sqrt((mu[0] - x[:, i]) ** 2 + (mu[1] - y[:, i]) ** 2) for mu in means], axis=0)
        live = np.nonzero(~(dist > 5.0))[0]
        if len(live) == 0:
            continue
        cov = covs[i - 1]
        if np.all(cov == 0):
            cov = np.array([[0.1, 0.0], [0.0, 0.1]])
        sx, sy = np.sqrt(cov[0, 0]), np.sqrt(cov[1, 1])
        r = cov[1, 0] / sy / sx
        cx, cy, t = x[live, i], y[live, i], th[live, i]
        rx = (ego_length / 2) * (2 / 3)
        centres = [(cx, cy), (cx + rx * np.cos(t), cy + rx * np.sin(t)), (cx - rx * np.cos(t), cy - rx * np.sin(t))]
        p = np.zeros(len(live))
        for mu in means:
            for (ccx, ccy) in centres:
                a1, a2 = ((ccx - off[0]) - mu[0]) / sx, ((ccy - off[1]) - mu[1]) / sy
                b1, b2 = ((ccx + off[0]) - mu[0]) / sx, ((ccy + off[1]) - mu[1]) / sy
                p = p + (((rr.bvnu(a1, a2, r) - rr.bvnu(b1, a2, r)) - rr.bvnu(a1, b2, r)) + rr.bvnu(b1, b2, r))
        prob[live, i - 1] = p / 3
    return prob


def calc_risk_detail(x, y, th, v, predictions, types, modes, coeff, ego_length, ego_width, ego_mass):
    """calc_risk's seven results: dict of ego_risk_max, obst_risk_max, ego_harm_max, obst_harm_max [C, K], ego_risk, obst_risk,
    obst_harm_occ [C].  An obstacle with min(L - 1, len(pos_list)) == 0 raises ValueError (np.max of an empty list upstream)."""
    x, y, th, v = (np.atleast_2d(np.asarray(a, np.float64)) for a in (x, y, th, v))
    C, L = x.shape
    K = len(predictions)
    out = {n: np.zeros((C, K)) for n in ("ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max")}
    occ = np.zeros((C, K))
    for k, (oid, pr) in enumerate(predictions.items()):
        if min(L - 1, len(pr["pos_list"])) == 0:
            raise ValueError(f"obstacle {oid}: empty harm list (np.max of an empty list upstream)")
        e, o = rr.calc_risk(x, y, th, v, {oid: pr}, types, modes, coeff, ego_length, ego_width, ego_mass)
        out["ego_risk_max"][:, k], out["obst_risk_max"][:, k] = e, o
        key = str(types[oid]).replace("_", "").lower()
        he, ho = _harm(x, y, th, v, pr, key, modes, coeff, ego_mass)
        out["ego_harm_max"][:, k], out["obst_harm_max"][:, k] = he.max(axis=1), ho.max(axis=1)
        prob = probability(x, y, th, pr, modes, ego_length, ego_width)
        am = np.argmax(prob, axis=1)   # first maximum (risk_costs.py:104-107)
        hit = prob.max(axis=1) > 0.001
        occ[:, k] = np.where(hit, ho[np.arange(C), np.minimum(am, ho.shape[1] - 1)], 0.0)
    if K:
        out["ego_risk"], out["obst_risk"] = out["ego_risk_max"].max(axis=1), out["obst_risk_max"].max(axis=1)
        out["obst_harm_occ"] = occ.max(axis=1)
    else:
        out["ego_risk"] = out["obst_risk"] = out["obst_harm_occ"] = np.zeros(C)
    return out


# ---- risk_costs.py:124-222, one trajectory: lists in obstacle order -------------------------------------------------------

def bayesian(ego_risk_max, obst_risk_max, boundary_harm):
    if len(ego_risk_max) == 0:
        return 0
    return (sum(ego_risk_max) + sum(obst_risk_max) + boundary_harm) / (len(ego_risk_max) * 2)


def equality(ego_risk_max, obst_risk_max):
    if len(ego_risk_max) == 0:
        return 0
    return sum([abs(a - b) for a, b in zip(ego_risk_max, obst_risk_max)]) / len(ego_risk_max)


def maximin(ego_risk_max, obst_risk_max, ego_harm_max, obst_harm_max, boundary_harm, eps=10e-10, scale_factor=10):
    if len(ego_harm_max) == 0:
        return 0
    # upstream's gate, kept: the harm survives where the risk is BELOW eps
    maximin_ego = [a * int(b < eps) for a, b in zip(ego_harm_max, ego_risk_max)]
    maximin_obst = [a * int(bool(b < eps)) for a, b in zip(obst_harm_max, obst_risk_max)]
    return max(maximin_ego + maximin_obst + [boundary_harm]) ** scale_factor


def ego_cost(ego_risk_max, boundary_harm):
    if len(ego_risk_max) == 0:
        return 0
    return sum(ego_risk_max) + boundary_harm


# ---- utility/responsibility.py ----------------------------------------------------------------------------------------------

def inside180view(ego_position, ego_orientation, prediction):
    dx = prediction["pos_list"][0][0] - ego_position[0]
    dy = prediction["pos_list"][0][1] - ego_position[1]
    a = np.arctan2(dy, dx)
    return bool(ego_orientation - (np.pi / 4) <= a <= ego_orientation + (np.pi / 4))


def responsibility_action_space(obst_risk_max, predictions, ego_position, ego_orientation):
    cost = 0
    for k, oid in enumerate(predictions):
        cost -= (0 if inside180view(ego_position, ego_orientation, predictions[oid]) else 1) * obst_risk_max[k]
    return cost


def polygon_padding(max_len, polys):
    res = np.zeros((len(polys), max_len, 2))
    for i, p in enumerate(polys):
        res[i][:len(p)] = p
        if len(p) < max_len:
            res[i][len(p):] = p[-1]
    return res


def contains(poly, px, py):
    """strict interior by the even-odd crossing rule (ray towards +x); poly [m, 2], closed or not"""
    inside = False
    m = len(poly)
    for i in range(m):
        xi, yi = poly[i]
        xj, yj = poly[i - 1]
        if (yi > py) != (yj > py) and px < (xj - xi) * (py - yi) / (yj - yi) + xi:
            inside = not inside
    return inside


def time_steps(time_t, dt):
    """the reference's own expression (its truncation kept: 0.3 / 0.1 - 1 -> 1)"""
    return np.array(np.asarray(time_t) / dt - 1, dtype=int)


def responsibility_reach_set(x, y, dt, reach_sets, obst_risk_max, keys):
    """calc_responsibility_reach_set for ONE trajectory (x, y [L]); obst_risk_max in the order of `keys`.  Returns the cost and
    the containment lists (bool_contain_cache).  ValueError where upstream raises KeyError / IndexError."""
    index = {oid: k for k, oid in enumerate(keys)}
    cost = 0.0
    cache = []
    for oid, rs in reach_sets.items():
        if oid not in index:
            raise ValueError(f"reach-set obstacle {oid} is not in the predictions")
        time_t = np.array([list(part.keys())[0] for part in rs])
        steps = time_steps(time_t, dt)
        polys = [np.asarray(list(part.values())[0], np.float64) for part in rs]
        padded = polygon_padding(max(len(p) for p in polys), polys)
        mask = np.array(time_t > 0, dtype=int)
        if np.any((steps >= len(x)) & (mask == 1)):
            raise ValueError(f"reach-set obstacle {oid}: step index outside the trajectory")
        inside = np.array([contains(padded[i], x[steps[i]], y[steps[i]]) for i in range(len(rs))], dtype=int)   # (-1 wraps, as upstream)
        cache.append(inside)
        if 1 not in inside * mask:
            cost -= obst_risk_max[index[oid]]
    return cost, cache


def costs(detail, boundary_harm, weights, resp=None):
    """The five principles [C] and their weighted total from calc_risk_detail's dict; resp: [C] responsibility costs or None"""
    C, K = detail["ego_risk_max"].shape
    bh = np.broadcast_to(np.asarray(boundary_harm, np.float64), (C,))
    out = {n: np.zeros(C) for n in NAMES}
    for c in range(C):
        er, orr = list(detail["ego_risk_max"][c]), list(detail["obst_risk_max"][c])
        eh, oh = list(detail["ego_harm_max"][c]), list(detail["obst_harm_max"][c])
        out["bayes"][c] = bayesian(er, orr, bh[c])
        out["equality"][c] = equality(er, orr)
        out["maximin"][c] = maximin(er, orr, eh, oh, bh[c])
        out["ego"][c] = ego_cost(er, bh[c])
    if resp is not None and K > 0:
        out["responsibility"] = np.asarray(resp, np.float64)
    out["total"] = sum(w * out[n] for w, n in zip(weights, NAMES))
    return out


def argmin_index(total, ids):
    """first minimum over the comparable totals in candidate order, -1 when there is none"""
    total = np.asarray(total, np.float64)
    ok = ~np.isnan(total)
    if not ok.any():
        return -1
    j = np.nonzero(ok)[0]
    return int(np.asarray(ids)[j[int(np.argmin(total[j]))]])


def near_discontinuity(planes, preds, modes, ego_risk_max, obst_risk_max, ego_length, ego_width, ego_mass=None, eps=10e-10):
    """[n] candidates a perturbation of 1e-9 in the planes may move across a decision: the rule of test_risk_golden (5 m gate,
    impact-area edges), a per-obstacle risk within 1e-6 (relative) of the maximin gate's eps, a probability maximum within 1e-9
    of obst_harm_occ's 0.001.  planes [n, 4, L]."""
    from tests.test_risk_golden import _near_discontinuity
    near = _near_discontinuity(planes, preds, modes)
    for a in (ego_risk_max, obst_risk_max):
        near |= np.any(np.abs(np.asarray(a) - eps) <= 1e-6 * eps, axis=1)
    for pr in preds.values():
        prob = probability(planes[:, 0], planes[:, 1], planes[:, 2], pr, modes, ego_length, ego_width)
        near |= np.abs(prob.max(axis=1) - 0.001) <= 1e-9
    return near


def load_golden(name):
    """(golden, source risk golden, predictions, types, reach sets {id: [{time_t: polygon}]}, variants) of tests/golden/<name>.npz"""
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    src = dict(np.load(os.path.join(GOLDEN, str(g["source"]) + ".npz")))
    keys = [int(k) for k in src["pred_keys"]]
    preds = {k: dict(pos_list=src["pred_pos"][j], cov_list=src["pred_cov"][j], orientation_list=src["pred_yaw"][j],
                     v_list=src["pred_v"][j], shape=dict(length=float(src["pred_shape"][j][0]), width=float(src["pred_shape"][j][1])))
             for j, k in enumerate(keys)}
    types = {k: str(t) for k, t in zip(keys, src["pred_types"])}
    sets, p, v = {}, 0, 0
    for oid, cnt in zip(g["rs_keys"], g["rs_entry_parts"]):
        parts = []
        for _ in range(int(cnt)):
            m = int(g["rs_vert_count"][p])
            parts.append({float(g["rs_time_t"][p]): g["rs_verts"][v:v + m].copy()})
            p, v = p + 1, v + m
        sets[int(oid)] = parts
    variants = [json.loads(str(x)) for x in g["variants"]]
    return g, src, preds, types, sets, variants
