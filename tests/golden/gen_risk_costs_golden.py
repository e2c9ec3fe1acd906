"""Generate tests/golden/risk_costs_*.npz: the reference's own `calc_risk` (all seven results), `get_bayesian_costs`,
`get_equality_costs`, `get_maximin_costs`, `get_ego_costs` and `get_responsibility_cost` in both modes
(risk_assessment/risk_costs.py, frenetix_motion_planner/utility/responsibility.py) on the trajectories of the risk goldens.

Run from the repository root with the reference tree present:  python tests/golden/gen_risk_costs_golden.py

Trajectories, predictions, obstacle types and the three shims (ObstacleType, RectOBB, mvnun) are gen_risk_golden.py's.  A fourth
shim stands in for `pygeos`, which is not installed here: `points` and `polygons` keep the coordinate arrays, `contains` is the
strict interior by the even-odd crossing rule.  Parity of that rule with pygeos on points ON an edge is
unpinned; the generator asserts that no tested point lies within 1e-3 m of an edge, where the two cannot differ.

Three variants per file (default, ignore_angle, Mahalanobis).  boundary_harm is a stored mix of zeros and logistic values.  The
reach sets are synthetic: convex polygons growing along each prediction (unequal vertex counts, so that upstream pads them), one
concave L-shape, a sparse time_t list that includes 0.3 (0.3 / 0.1 - 1 truncates to step 1) and one time_t = 0 part that
contains every tested point and must be ignored.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import gen_risk_golden as base  # noqa: E402
from tests import risk_costs_restatement as rcr  # noqa: E402

WEIGHTS = [1.0, 0.5, 2.0, 0.25, 1.5]   # bayes, equality, maximin, ego, responsibility
TIME_T = [0.0, 0.3, 0.5, 1.0, 1.6, 2.2, 2.9]
ORIENTATION_OFFSET = 0.5   # rad on top of the trajectories' initial heading: obstacles on both sides of the +-pi/4 view
BOUNDARY = (-4.591, 0.185)   # harm_parameters.json log_reg.ignore_angle const / speed


def install_pygeos_shim():
    mod = types.ModuleType("pygeos")
    mod.points = lambda coords, *a: np.asarray(coords, np.float64)
    mod.polygons = lambda rings: np.asarray(rings, np.float64)
    mod.contains = lambda polys, pts: np.array([rcr.contains(p, q[0], q[1]) for p, q in zip(polys, pts)])
    sys.modules["pygeos"] = mod


def variants():
    return [dict(base.MODES), dict(base.MODES, ignore_angle=True, sym_angle=False, reduced_angle_areas=False),
            dict(base.MODES, fast_prob_mahalanobis=True)]


def ngon(centre, radius, m, phase):
    a = phase + 2 * np.pi * np.arange(m) / m
    return np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1)


def l_shape(centre, size):
    """concave: a square with its upper right quarter cut away"""
    s = size
    pts = np.array([[-s, -s], [s, -s], [s, 0.0], [0.0, 0.0], [0.0, s], [-s, s]])
    return pts + np.asarray(centre)


def reach_sets_for(keys, preds, planes, dt, shift=0.0):
    """obstacle id -> list of {time_t: polygon}.  Obstacle 0's polygons sit on the candidates' own points so that both containment
    outcomes occur; obstacle 1 (if any) carries the L-shape; the others grow along their prediction."""
    out = {}
    steps = rcr.time_steps(np.array(TIME_T), dt)
    for n, oid in enumerate(keys[:6]):
        pos = np.asarray(preds[oid]["pos_list"])
        parts = []
        for ti, (t, st) in enumerate(zip(TIME_T, steps)):
            if t <= 0:
                if n == 0:   # contains every point of every trajectory: only the time_t > 0 mask keeps it out
                    c = planes[:, :2, :].mean(axis=(0, 2))
                    parts.append({t: ngon(c, 1.0e4, 4, 0.3)})
                continue
            pts = planes[:, :2, st]
            spread = max(np.ptp(pts[:, 0]), np.ptp(pts[:, 1]), 0.5)
            if n == 0:   # two small polygons on the candidates' own points: inside for some candidates, outside for the others
                if ti >= 5:
                    parts.append({t: ngon(np.median(pts, axis=0) + np.array([0.13 + shift, -0.07]), 0.2 * spread + 0.11, 4 + ti % 5, 0.1 * ti)})
                continue
            if n == 1 and ti == 3:
                parts.append({t: l_shape(np.median(pts, axis=0) + np.array([0.21, 0.17 + shift]), 0.25 * spread + 0.1)})
                continue
            if (ti + n) % 3 == 2:
                continue   # sparse, different per obstacle
            parts.append({t: ngon(pos[min(st, len(pos) - 1)], 1.0 + 0.8 * t, 4 + (ti + n) % 5, 0.2 * n + 0.1 * ti)})
        out[oid] = parts
    return out


def edge_distance(poly, px, py):
    d = np.inf
    for i in range(len(poly)):
        a, b = poly[i - 1], poly[i]
        ab = b - a
        L2 = float(ab @ ab)
        u = 0.0 if L2 == 0 else float(np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / L2, 0, 1))
        d = min(d, np.hypot(px - (a[0] + u * ab[0]), py - (a[1] + u * ab[1])))
    return d


def main():
    ObstacleType = base.install_shims()
    install_pygeos_shim()
    from risk_assessment.risk_costs import (calc_risk, get_bayesian_costs, get_equality_costs, get_maximin_costs, get_ego_costs,
                                            get_responsibility_cost)
    params_harm = json.load(open(os.path.join(HERE, "harm_parameters.json")))
    veh = types.SimpleNamespace(**base.EGO)
    for name, src, tnames in base.SCENARIOS:
        g = np.load(os.path.join(HERE, src))
        dt = float(g["dt"])
        keys = [int(k) for k in g["pred_keys"]]
        preds = {}
        for j, oid in enumerate(keys):
            pos = g["pred_pos"][j]
            step = np.sqrt(np.sum(np.diff(pos, axis=0) ** 2, axis=1)) / dt
            preds[oid] = dict(pos_list=pos.copy(), cov_list=g["pred_cov"][j].copy(), orientation_list=g["pred_yaw"][j].copy(),
                              v_list=np.append(step, step[-1] if len(step) else 0.0),
                              shape=dict(length=float(g["pred_shape"][j][0]), width=float(g["pred_shape"][j][1])))
        types_ = {oid: getattr(ObstacleType, t) for oid, t in zip(keys, tnames)}
        scenario = types.SimpleNamespace(obstacle_by_id=lambda oid, _t=types_: types.SimpleNamespace(obstacle_type=_t[oid]))
        keep = g["has_cart"][g["plane_ids"]]
        ids = np.asarray(g["plane_ids"], np.int64)[keep]
        planes = g["planes"][keep][:, :4, :]
        n, K = len(ids), len(keys)
        # stored boundary harm: every third candidate leaves the road at a step of its own
        bh = np.zeros(n)
        for c in range(0, n, 3):
            bh[c] = 1.0 / (1.0 + np.exp(-BOUNDARY[0] - BOUNDARY[1] * planes[c, 3, 3 + c % 20]))
        ego_state = types.SimpleNamespace(position=planes[0, :2, 0].copy(), orientation=float(planes[0, 2, 0]) + ORIENTATION_OFFSET, time_step=7)
        # every tested point at least 1e-3 m away from every polygon edge: the first shift of the synthetic polygons that gives it
        for shift in np.arange(0.0, 0.2, 0.011):
            sets = reach_sets_for(keys, preds, planes, dt, shift)
            dmin = np.inf
            for oid, parts in sets.items():
                for part in parts:
                    (t, poly), = part.items()
                    if t > 0:
                        st = int(rcr.time_steps(np.array([t]), dt)[0])
                        dmin = min(dmin, min(edge_distance(poly, planes[c, 0, st], planes[c, 1, st]) for c in range(n)))
            if dmin >= 1e-3:
                break
        reach = types.SimpleNamespace(reach_sets={7: sets})
        assert dmin >= 1e-3, (name, dmin)
        rs_keys = list(sets)
        out = dict(plane_ids=ids, boundary_harm=bh, ego_position=ego_state.position, ego_orientation=np.float64(ego_state.orientation),
                   dt=np.float64(dt), weights=np.array(WEIGHTS), rs_keys=np.array(rs_keys),
                   rs_entry_parts=np.array([len(sets[k]) for k in rs_keys]),
                   rs_time_t=np.array([list(p.keys())[0] for k in rs_keys for p in sets[k]]),
                   rs_vert_count=np.array([len(list(p.values())[0]) for k in rs_keys for p in sets[k]]),
                   rs_verts=np.concatenate([list(p.values())[0] for k in rs_keys for p in sets[k]]),
                   source=np.array(name.replace("risk_costs_", "risk_")))
        names = []
        for vi, modes in enumerate(variants()):
            tag = f"v{vi}"
            cols = {q: np.zeros((n, K)) for q in ("ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max")}
            sc = {q: np.zeros(n) for q in ("ego_risk", "obst_risk", "obst_harm_occ", "bayes", "equality", "maximin", "ego", "resp_action",
                                           "resp_reach")}
            contain = []
            for c in range(n):
                traj = types.SimpleNamespace(dt=dt, cartesian=types.SimpleNamespace(x=planes[c, 0], y=planes[c, 1], theta=planes[c, 2],
                                                                                   v=planes[c, 3]))
                r = calc_risk(traj, ego_state, preds, scenario, 24, veh, params_harm, modes)
                for q, d in zip(("ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max"), r[:4]):
                    assert list(d.keys()) == keys
                    cols[q][c] = [d[k] for k in keys]
                sc["ego_risk"][c], sc["obst_risk"][c], sc["obst_harm_occ"][c] = r[4], r[5], r[6]
                sc["bayes"][c] = get_bayesian_costs(r[0], r[1], bh[c])
                sc["equality"][c] = get_equality_costs(r[0], r[1])
                sc["maximin"][c] = get_maximin_costs(r[0], r[1], r[2], r[3], bh[c])
                sc["ego"][c] = get_ego_costs(r[0], bh[c])
                pr2 = {k: dict(v) for k, v in preds.items()}   # (the action-space mode writes 'responsibility' into them)
                sc["resp_action"][c], _ = get_responsibility_cost(scenario, traj, ego_state, r[1], pr2, None, mode="action_space")
                sc["resp_reach"][c], cache = get_responsibility_cost(scenario, traj, ego_state, r[1], preds, reach, mode="reach_set")
                contain.append(np.concatenate(cache))
            contain = np.array(contain, dtype=np.int8)
            # both containment outcomes among the parts that count
            live = out["rs_time_t"] > 0
            assert contain[:, live].any() and not contain[:, live].all(), name
            # ... and for the decision of an entry: some obstacle is subtracted for some candidates and not for others
            first = np.concatenate([[0], np.cumsum(out["rs_entry_parts"])])
            hit = np.array([(contain[:, a:b] * live[a:b]).any(axis=1) for a, b in zip(first[:-1], first[1:])])   # [entries, n]
            assert (hit.any(axis=1) & ~hit.all(axis=1)).sum() >= 2, (name, hit.sum(axis=1))
            for q, a in {**cols, **sc}.items():
                out[f"{tag}_{q}"] = a
            out[tag + "_contain"] = contain
            for mode in ("action", "reach"):
                p5 = [sc["bayes"], sc["equality"], sc["maximin"], sc["ego"], sc["resp_" + mode]]
                total = sum(w * p for w, p in zip(WEIGHTS, p5))
                out[f"{tag}_total_{mode}"] = total
                out[f"{tag}_min_index_{mode}"] = np.int64(ids[int(np.argmin(total))])
            near = rcr.near_discontinuity(planes, preds, modes, cols["ego_risk_max"], cols["obst_risk_max"], *base.EGO.values())
            assert near.mean() < 0.05, (name, tag, near.mean())
            names.append(json.dumps(dict(modes, obstacles=keys)))
            print(f"  {name} {tag}: candidates inside a part, per reach-set obstacle: {hit.sum(axis=1)} of {n}, "
                  f"{int(near.sum())} near a discontinuity, min edge distance {dmin:.3g} m")
        out["variants"] = np.array(names)
        # the responsibility vector the action-space mode assigned (both values should occur in at least one file)
        out["resp_vector"] = np.array([0.0 if rcr.inside180view(ego_state.position, ego_state.orientation, preds[k]) else 1.0 for k in keys])
        assert 0 < out["resp_vector"].sum() < K, (name, out["resp_vector"])
        path = os.path.join(HERE, name.replace("risk_", "risk_costs_") + ".npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {n} trajectories x {len(names)} variants, {os.path.getsize(path)} bytes, resp vector {out['resp_vector']}")


if __name__ == "__main__":
    main()
