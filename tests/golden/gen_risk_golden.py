"""Generate tests/golden/risk_*.npz: the reference's own `calc_risk` (risk_assessment/risk_costs.py) on trajectories the
reference planner produced.

Run from the repository root with the reference tree present:  python tests/golden/gen_risk_golden.py

Inputs: the reference trajectories stored in existing goldens (their `planes` are the cartesian x, y, theta, v of the
candidates `run_reference` returned -- gen_golden.py) and their predictions; `v_list` (absent from those goldens) is the
obstacle's speed along its predicted positions, |pos[i+1] - pos[i]| / dt (last value repeated).  Obstacle types are assigned
per scenario (car / truck / pedestrian / bicycle ...).  For every variant of risk.json / harm_parameters.json the reference's
`calc_risk` runs on every stored trajectory; the variants it cannot evaluate are not stored.

Three shims, because the reference's dependencies are not installed here:
  * commonroad.scenario.obstacle.ObstacleType -- a real Enum.  ref_harness's permissive stub would make every member the same
    object, so every key of harm_estimation.obstacle_protection would collapse into one.
  * commonroad_dc.pycrcc.RectOBB(r_x, r_y, theta, x, y) -- center() = (x, y), r_x() = the first half extent,
    local_x_axis() = (cos theta, sin theta): what collision_probability.get_center_points_for_shape_estimation reads.
  * scipy.stats.mvn.mvnun -- gone from the installed SciPy (the reference locks 1.13.1).  Replaced by a deterministic
    rectangle probability through Owen's T (scipy.special.owens_t; tests/risk_restatement.rect_probability_owens), an
    algorithm independent of the Genz BVNU the kernel uses.  Unverified: that SciPy 1.13's two-dimensional mvnun is Genz's
    deterministic routine rather than a lattice rule; the agreement targets do not depend on it.
"""
import enum
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_harness  # noqa: E402
from tests import risk_restatement as rr  # noqa: E402

TYPE_NAMES = ["CAR", "TRUCK", "BUS", "BICYCLE", "PEDESTRIAN", "PRIORITY_VEHICLE", "PARKED_VEHICLE", "TRAIN", "MOTORCYCLE", "TAXI",
              "ROAD_BOUNDARY", "PILLAR", "CONSTRUCTION_ZONE", "BUILDING", "MEDIAN_STRIP", "UNKNOWN"]
COMMONROAD_NAME = {"CAR": "car", "TRUCK": "truck", "BUS": "bus", "BICYCLE": "bicycle", "PEDESTRIAN": "pedestrian",
                   "PRIORITY_VEHICLE": "priorityVehicle", "PARKED_VEHICLE": "parkedVehicle", "TRAIN": "train",
                   "MOTORCYCLE": "motorcycle", "TAXI": "taxi", "UNKNOWN": "unknown"}
EGO = dict(length=4.508, width=1.61, mass=1239.0)   # (BMW 320i of commonroad-vehicle-models, vehicle type 2)


def install_shims():
    ref_harness.install()
    ObstacleType = enum.Enum("ObstacleType", {n: COMMONROAD_NAME.get(n, n.lower()) for n in TYPE_NAMES})
    mod = types.ModuleType("commonroad.scenario.obstacle")
    mod.ObstacleType = ObstacleType
    import commonroad.scenario  # noqa: F401  (stub package)
    sys.modules["commonroad.scenario.obstacle"] = mod

    class RectOBB:
        def __init__(self, r_x, r_y, theta, x, y):
            self._rx, self._ry, self._th, self._c = r_x, r_y, theta, np.array([x, y], dtype=np.float64)

        def center(self):
            return self._c.copy()

        def r_x(self):
            return self._rx

        def local_x_axis(self):
            return np.array([np.cos(self._th), np.sin(self._th)])
    pycrcc = types.ModuleType("commonroad_dc.pycrcc")
    pycrcc.RectOBB = RectOBB
    import commonroad_dc  # noqa: F401  (stub package)
    sys.modules["commonroad_dc.pycrcc"] = pycrcc
    sys.modules["commonroad_dc"].pycrcc = pycrcc

    import scipy.stats
    mvn = types.ModuleType("scipy.stats.mvn")
    mvn.mvnun = lambda lower, upper, means, covar, *a, **k: (rr.rect_probability_owens(lower, upper, means, covar), 0)
    scipy.stats.mvn = mvn
    sys.modules["scipy.stats.mvn"] = mvn
    return ObstacleType


SCENARIOS = [
    # (output, source golden, obstacle types in prediction order)
    ("risk_obs5", "arc_hv_l2_debug_obs5.npz", ["CAR", "CAR", "TRUCK", "CAR", "BUS"]),
    ("risk_mixed_obs6", "arc_hv_l3_prod_obs6.npz", ["CAR", "TRUCK", "PEDESTRIAN", "BICYCLE", "MOTORCYCLE", "TAXI"]),
    ("risk_config3_obs20", "config3_grid_prod_obs20.npz", ["CAR"] * 20),
]

MODES = dict(harm_mode="log_reg", ignore_angle=False, sym_angle=True, reduced_angle_areas=True, crash_angle_simplified=True,
             fast_prob_mahalanobis=False)


def variants():
    out = []
    for ign in (False, True):
        for sym in (False, True):
            for red in (False, True):
                if ign and (sym or red):
                    continue
                out.append(dict(MODES, ignore_angle=ign, sym_angle=sym, reduced_angle_areas=red))
    out.append(dict(MODES, harm_mode="ref_speed", ignore_angle=True))
    out.append(dict(MODES, harm_mode="gidas"))              # unprotected obstacles only
    out.append(dict(MODES, fast_prob_mahalanobis=True))
    return out


def main():
    ObstacleType = install_shims()
    from risk_assessment.risk_costs import calc_risk
    import json
    params_harm = json.load(open(os.path.join(HERE, "harm_parameters.json")))
    veh = types.SimpleNamespace(**EGO)
    for name, src, tnames in SCENARIOS:
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
        keep = g["has_cart"][g["plane_ids"]]          # rows the reference returned a cartesian trajectory for (others are zeros)
        ids = np.asarray(g["plane_ids"], np.int64)[keep]
        planes = g["planes"][keep][:, :4, :]   # x, y, theta, v
        out = dict(plane_ids=ids, planes=planes, pred_keys=np.array(keys), pred_types=np.array([COMMONROAD_NAME[t] for t in tnames]),
                   pred_pos=g["pred_pos"], pred_cov=g["pred_cov"], pred_yaw=g["pred_yaw"], pred_shape=g["pred_shape"],
                   pred_v=np.stack([preds[k]["v_list"] for k in keys]), ego=np.array([EGO["length"], EGO["width"], EGO["mass"]]))
        names = []
        t_total, n_total = 0.0, 0
        for vi, modes in enumerate(variants()):
            if modes["harm_mode"] == "gidas" and any(rr.PROTECTION[COMMONROAD_NAME[t].lower()] for t in tnames):
                # gidas only for unprotected obstacles: the pedestrian / bicycle / motorcycle subset of the scenario
                sub = [k for k, t in zip(keys, tnames) if not rr.PROTECTION[COMMONROAD_NAME[t].lower()]]
                if not sub:
                    continue
            else:
                sub = keys
            if modes["harm_mode"] == "ref_speed" and not modes["ignore_angle"]:
                continue
            pr = {k: preds[k] for k in sub}
            ego_r, obst_r = np.zeros(len(ids)), np.zeros(len(ids))
            t0 = time.perf_counter()
            for c in range(len(ids)):
                traj = types.SimpleNamespace(cartesian=types.SimpleNamespace(x=planes[c, 0], y=planes[c, 1], theta=planes[c, 2],
                                                                            v=planes[c, 3]))
                r = calc_risk(traj, None, pr, scenario, 24, veh, params_harm, modes)
                ego_r[c], obst_r[c] = r[4], r[5]
            t_total += time.perf_counter() - t0
            n_total += len(ids)
            tag = f"v{vi}"
            names.append(json.dumps(dict(modes, obstacles=sub)))
            out[tag + "_ego"] = ego_r
            out[tag + "_obst"] = obst_r
            s = ego_r + obst_r
            out[tag + "_min_index"] = np.int64(ids[int(np.argmin(s))])   # sorted(..., key=ego + obst)[0]: first minimum
        out["variants"] = np.array(names)
        out["ref_seconds_per_trajectory"] = np.float64(t_total / max(n_total, 1))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {len(ids)} trajectories x {len(names)} variants, {os.path.getsize(path)} bytes, "
              f"reference calc_risk {1e3 * t_total / max(n_total, 1):.2f} ms per trajectory")


if __name__ == "__main__":
    main()
