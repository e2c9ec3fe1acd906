"""What the risk-family test modules share of their scenes: the harm parameters and model switches, obstacles that walk along an
agent's own candidates, synthetic reach sets, per-agent ego dimensions and weights, and the error measure of the restatement
comparisons.  No test lives here; the modules import these (some under the private names they had when each module had its own)."""
import json
import os

import numpy as np

from tests import risk_costs_restatement as rcr

HARM = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "harm_parameters.json")))
BASE = dict(harm_mode="log_reg", ignore_angle=False, sym_angle=True, reduced_angle_areas=True, crash_angle_simplified=True,
            fast_prob_mahalanobis=False)
# the model switches of a batch's agents, by agent (modulo 5)
MODES = [BASE, BASE, BASE, dict(BASE, fast_prob_mahalanobis=True), dict(BASE, harm_mode="ref_speed", ignore_angle=True)]


def predictions(planes, flags, rng, n_obs=8, types=None, zero_cov=True):
    """Obstacles that walk along (shifted) ego candidates, so that many (candidate, obstacle, step) triples pass the 5 m gate,
    with covariances whose correlations cover every branch of the bivariate normal (0, < 0.3, < 0.75, < 0.925, >= 0.925),
    zero covariances and predictions shorter than the horizon."""
    from frenetix_motion_planner_amd import _abi
    C, S = planes["x"].shape
    ok = np.nonzero((flags & 0xB) == 0xB)[0]
    preds, typ = {}, {}
    rhos = [0.0, 0.2, -0.6, 0.8, -0.95, 0.99, 0.5, -0.1]
    kinds = types or ["car", "truck", "pedestrian", "bicycle", "car", "bus", "motorcycle", "car"]
    for k in range(n_obs):
        c = ok[rng.integers(len(ok))]
        P = S - 1 if k % 3 else S - 7
        off = rng.normal(0, 1.0, 2)
        pos = np.stack([planes["x"][c, :P] + off[0], planes["y"][c, :P] + off[1]], axis=1)
        r = rhos[k % len(rhos)]
        sx, sy = 0.3 + 0.1 * k, 0.5
        cov = np.tile(np.array([[sx * sx, r * sx * sy], [r * sx * sy, sy * sy]]), (P, 1, 1)) * np.linspace(1, 3, P)[:, None, None]
        if k == 2 and zero_cov:   # (all-zero covariances become 0.1 I in the default mode; np.linalg.inv refuses them)
            cov[:4] = 0.0
        preds[100 + k] = dict(pos_list=pos, cov_list=cov, orientation_list=planes["theta"][c, :P] + rng.normal(0, 0.5),
                              v_list=np.abs(planes["v"][c, :P] + rng.normal(0, 2)), shape=dict(length=4.0 + 0.3 * k, width=1.8))
        typ[100 + k] = kinds[k % len(kinds)]
    return preds, typ



def err(got, want):
    return float((np.abs(got - want) / np.maximum(np.abs(want), 1.0)).max()) if np.size(want) else 0.0


def reach_sets(planes, keys, sub, dt):
    """Synthetic reach sets on the candidates' own points (both outcomes occur), on the first obstacles: unequal vertex counts, a
    concave L, time_t 0.3 (step 1), a time_t = 0 part around everything, an obstacle whose only part is masked."""
    sets = {}
    for n, oid in enumerate(keys[:4]):
        parts = []
        if n == 0:
            parts.append({0.0: np.array([[-1e4, -1e4], [1e4, -1e4], [1e4, 1e4], [-1e4, 1e4]])})
        for ti, t in enumerate((0.3, 1.0, 2.2) if n < 3 else ()):
            st = int(rcr.time_steps([t], dt)[0])
            pts = np.stack([planes["x"][sub, st], planes["y"][sub, st]], axis=1)
            c = np.median(pts, axis=0) + np.array([0.137 * (n + 1), -0.071 * (ti + 1)])
            r = 0.25 * max(np.ptp(pts[:, 0]), np.ptp(pts[:, 1]), 0.4) + 0.05 * ti
            if n == 1 and ti == 1:
                poly = np.array([[-r, -r], [r, -r], [r, 0.0], [0.0, 0.0], [0.0, r], [-r, r]]) + c
            else:
                a = 0.3 * n + 2 * np.pi * np.arange(4 + ti + n) / (4 + ti + n)
                poly = c + r * np.stack([np.cos(a), np.sin(a)], axis=1)
            parts.append({t: poly})
        if n == 3:
            parts.append({-0.1: np.array([[-1e4, -1e4], [1e4, -1e4], [1e4, 1e4], [-1e4, 1e4]])})
        sets[oid] = parts
    return sets



def ego(a):
    return dict(ego_length=4.508 + 0.1 * a, ego_width=1.61 + 0.02 * a, ego_mass=1239.0 + 50.0 * a)


def weight(a):
    return 0.5 + 0.1 * a


def resp_cost(resp):
    from frenetix_motion_planner_amd import risk
    return risk.risk_cost_params([0, 0, 0, 0, 1], responsibility=resp)

