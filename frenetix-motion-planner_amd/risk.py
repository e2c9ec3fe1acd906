"""Trajectory risk on the device: collision probability x harm (risk_costs.py:20-118 with crash_angle_simplified).

`risk_params` turns the reference's `risk.json` / `harm_parameters.json` dicts into the FxRiskParams block the kernel reads,
following `get_model` (harm_estimation.py) for every harm mode, protection class and angle variant; `obstacle_tables` packs
the predictions dict of a plan step into the per-obstacle tables of `fx_set_risk_obstacles_agent`.  DESIGN.md section 11.

`risk_cost_params`, `action_space_responsibility` and `reach_set_tables` prepare the risk-cost principles and the two
responsibility modes (risk_costs.py:124-251, utility/responsibility.py) of `fx_eval_risk_costs_agent`.  DESIGN.md section 13.
"""
import numpy as np

from . import _abi

# harm_estimation.py obstacle_protection (ObstacleType -> crash structure), keyed by the CommonRoad type name
PROTECTION = {"car": True, "truck": True, "bus": True, "bicycle": False, "pedestrian": False, "priorityvehicle": True,
              "parkedvehicle": True, "train": True, "motorcycle": False, "taxi": True, "roadboundary": None, "pillar": None,
              "constructionzone": None, "building": None, "medianstrip": None, "unknown": False}
_SIZE_MASS = ("car", "priorityvehicle", "parkedvehicle", "taxi")
_FIXED_MASS = {"truck": 25000, "bus": 13000, "bicycle": 90, "pedestrian": 75, "train": 118800, "motorcycle": 250}


def type_key(obstacle_type) -> str:
    """'priorityVehicle', 'PRIORITY_VEHICLE', ObstacleType.PRIORITY_VEHICLE -> 'priorityvehicle'"""
    name = getattr(obstacle_type, "name", obstacle_type)
    key = str(name).replace("_", "").lower()
    if key not in PROTECTION:
        raise ValueError(f"unknown obstacle type {obstacle_type!r}")
    return key


def obstacle_mass(obstacle_type, size: float) -> float:
    """helpers/properties.py get_obstacle_mass"""
    key = type_key(obstacle_type)
    if key in _SIZE_MASS:
        return -1333.5 + 526.9 * np.power(size, 0.8)
    return _FIXED_MASS.get(key, 0)


def _check_modes(params_risk):
    if params_risk.get("crash_angle_simplified") is False:
        raise NotImplementedError("crash_angle_simplified: false needs the scenario geometry (calc_crash_angle); not supported")
    if params_risk.get("harm_mode") not in ("log_reg", "ref_speed", "gidas"):
        raise ValueError("Please select a valid mode for harm estimation (log_reg, ref_speed, gidas)")


def check_obstacle_classes(params_risk, classes):
    """The combinations the reference cannot evaluate raise here, as they raise upstream."""
    _check_modes(params_risk)
    for oid, prot in classes.items():
        if prot is None:
            raise ValueError(f"obstacle {oid}: its type has no protection class (road boundary, pillar, ...): calc_risk fails upstream")
        if prot and params_risk["harm_mode"] == "gidas":
            raise ValueError(f"obstacle {oid}: harm_mode 'gidas' with a protected obstacle (get_model returns an unbound model upstream)")
        if prot and params_risk["harm_mode"] == "ref_speed" and not params_risk["ignore_angle"]:
            raise ValueError(f"obstacle {oid}: harm_mode 'ref_speed' with impact areas and a protected obstacle fails upstream "
                             "(reference_speed_*symmetrical.py compare the whole velocity array / index a scalar)")


def risk_params(params_risk: dict, params_harm: dict, ego_length: float, ego_width: float, ego_mass: float) -> _abi.FxRiskParams:
    """FxRiskParams for risk.json `params_risk` and harm_parameters.json `params_harm`; the ego's mass comes from the caller's
    vehicle model (no default)."""
    _check_modes(params_risk)
    p = _abi.FxRiskParams()
    p.prob_mode = _abi.FX_RISK_PROB_MAHALANOBIS if params_risk.get("fast_prob_mahalanobis") else _abi.FX_RISK_PROB_MVN
    mode = params_risk["harm_mode"]
    ign, sym, red = bool(params_risk["ignore_angle"]), bool(params_risk["sym_angle"]), bool(params_risk["reduced_angle_areas"])
    p.prot_model = _abi.FX_RISK_HARM_LOGISTIC
    p.n_edges = 0
    if mode == "log_reg":
        if ign:
            blk = params_harm["log_reg"]["ignore_angle"]
        elif not red:
            # 12 impact areas: (-15, 15) deg front, then pairs of 30 deg bins, the rest (|a| >= 165 deg, unwrapped) area 6
            blk = params_harm["log_reg"]["complete_sym_angle_areas" if sym else "complete_angle_areas"]
            p.n_edges = 6
            for j, deg in enumerate((15, 45, 75, 105, 135, 165)):
                p.edges[j] = deg / 180 * np.pi
            if sym:
                names = ("Imp_1_11", "Imp_2_10", "Imp_3_9", "Imp_4_8", "Imp_5_7")
                for j, n in enumerate(names, 1):
                    p.coef_pos[j] = p.coef_neg[j] = blk[n]
            else:
                for j, (pos, neg) in enumerate((("Imp_11", "Imp_1"), ("Imp_10", "Imp_2"), ("Imp_9", "Imp_3"), ("Imp_8", "Imp_4"),
                                                ("Imp_7", "Imp_5")), 1):
                    p.coef_pos[j], p.coef_neg[j] = blk[pos], blk[neg]
            p.coef_else = blk["Imp_6"]
        else:
            blk = params_harm["log_reg"]["reduced_sym_angle_areas" if sym else "reduced_angle_areas"]
            p.n_edges = 2
            t_a = 45 / 180 * np.pi
            p.edges[0] = t_a
            p.edges[1] = 3 * t_a if sym else 135 / 180 * np.pi
            if sym:
                p.coef_pos[1] = p.coef_neg[1] = blk["side"]
            else:
                p.coef_pos[1], p.coef_neg[1] = blk["driver_side"], blk["right_side"]
            p.coef_else = blk["rear"]
        p.prot_c, p.prot_s = blk["const"], blk["speed"]
        lr = params_harm["log_reg"]["ignore_angle"]
        p.unprot_ego_model = _abi.FX_RISK_HARM_LOGISTIC
        p.uego_c, p.uego_s = lr["const"], lr["speed"]
        p.ped_c, p.ped_s = params_harm["pedestrian"]["const"], params_harm["pedestrian"]["speed"]
    elif mode == "ref_speed":
        rs = params_harm["ref_speed"]["ignore_angle"]
        p.prot_model = _abi.FX_RISK_HARM_REF_SPEED          # (impact-area variants: check_obstacle_classes refuses them)
        p.prot_ref, p.prot_exp = rs["ref_speed"], rs["exp"]
        p.unprot_ego_model = _abi.FX_RISK_HARM_REF_SPEED
        p.uego_ref, p.uego_exp = rs["ref_speed"], rs["exp"]
        p.ped_c, p.ped_s = params_harm["pedestrian"]["const"], params_harm["pedestrian"]["speed"]
    else:  # gidas (protected obstacles: check_obstacle_classes refuses them)
        g = params_harm["gidas"]
        p.prot_c, p.prot_s = g["const"], g["speed"]
        p.unprot_ego_model = _abi.FX_RISK_HARM_LOGISTIC
        p.uego_c, p.uego_s = g["const"], g["speed"]
        m2 = params_harm["pedestrian_MAIS2+"]
        p.ped_c, p.ped_s = m2["const"], m2["speed"]
    p.ego_length, p.ego_width, p.ego_mass = float(ego_length), float(ego_width), float(ego_mass)
    if not (p.ego_mass > 0):
        raise ValueError("ego_mass must be positive (the vehicle model's mass)")
    return p


def obstacle_tables(predictions: dict, obstacle_types: dict, mahalanobis: bool = False) -> dict:
    """The arrays of fx_set_risk_obstacles_agent for a predictions dict (keys in its order, as calc_risk iterates them).
    obstacle_types: id -> CommonRoad type name; a missing id is a ValueError."""
    keys = list(predictions.keys())
    K = len(keys)
    lens = []
    for oid in keys:
        if oid not in obstacle_types:
            raise ValueError(f"obstacle {oid} has no type (set_risk_model obstacle_types)")
        pr = predictions[oid]
        for name in ("pos_list", "cov_list", "orientation_list", "v_list", "shape"):
            if name not in pr:
                raise ValueError(f"obstacle {oid}: the prediction lacks {name!r}")
        lens.append((len(pr["pos_list"]), len(pr["orientation_list"]), len(pr["v_list"])))
    P = max([max(x) for x in lens] + [1])
    pos = np.zeros((K, P, 2))
    cov = np.zeros((K, P, 4))
    cov_inv = np.zeros((K, P, 4))
    yaw = np.zeros((K, P))
    vel = np.zeros((K, P))
    n = np.zeros((3, K), np.int32)
    length, width, mass = np.zeros(K), np.zeros(K), np.zeros(K)
    cls = np.zeros(K, np.int32)
    classes = {}
    for k, oid in enumerate(keys):
        pr = predictions[oid]
        npos, nyaw, nv = lens[k]
        n[:, k] = lens[k]
        pos[k, :npos] = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
        c = np.asarray(pr["cov_list"], np.float64).reshape(-1, 2, 2)
        cov[k, :len(c)] = c.reshape(-1, 4)
        if mahalanobis and len(c):
            cov_inv[k, :len(c)] = np.linalg.inv(c).reshape(-1, 4)   # collision_probability.py:280 (singular: LinAlgError, as upstream)
        yaw[k, :nyaw] = np.asarray(pr["orientation_list"], np.float64)
        vel[k, :nv] = np.asarray(pr["v_list"], np.float64)
        length[k], width[k] = pr["shape"]["length"], pr["shape"]["width"]
        key = type_key(obstacle_types[oid])
        classes[oid] = PROTECTION[key]
        mass[k] = obstacle_mass(key, length[k] * width[k])
        cls[k] = _abi.FX_RISK_CLASS_PROTECTED if PROTECTION[key] else _abi.FX_RISK_CLASS_UNPROTECTED
    return dict(K=K, P=P, pos=pos, cov=cov, cov_inv=cov_inv, yaw=yaw, v=vel, n_pos=n[0].copy(), n_yaw=n[1].copy(), n_v=n[2].copy(),
                length=length, width=width, mass=mass, cls=cls, classes=classes, keys=keys)


def action_space_responsibility(predictions: dict, ego_position, ego_orientation: float) -> np.ndarray:
    """[K] 0 / 1 in the order of the predictions' keys, as assign_responsibility_by_action_space sets it: 0 for an obstacle whose
    first predicted position lies within +-pi/4 of the ego's orientation (check_if_inside180view: no angle wrap), 1 otherwise."""
    out = np.zeros(len(predictions))
    for k, pr in enumerate(predictions.values()):
        pos = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
        dx = pos[0, 0] - ego_position[0]
        dy = pos[0, 1] - ego_position[1]
        angle = np.arctan2(dy, dx)
        inside = ego_orientation - (np.pi / 4) <= angle <= ego_orientation + (np.pi / 4)
        out[k] = 0.0 if inside else 1.0
    return out


def reach_set_tables(reach_sets: dict, prediction_keys, dt: float, n_steps=None) -> dict:
    """The arrays of fx_set_reach_sets_agent for `reach_set.reach_sets[time_step]`: obstacle id -> list of one-item dicts
    {time_t: polygon vertices [m][2]} (calc_responsibility_reach_set).  The ego step of a part is the reference's own expression
    np.array(time_t / dt - 1, dtype=int) -- its truncation kept: 0.3 / 0.1 - 1 -> 1; parts with time_t <= 0 are dropped (upstream
    masks them).  An obstacle that is not among `prediction_keys` (KeyError upstream), a step index >= n_steps (IndexError
    upstream) and a polygon of fewer than 3 vertices raise ValueError."""
    index = {oid: k for k, oid in enumerate(prediction_keys)}
    entry_obs, entry_off, part_step, part_obs, vert_off, verts, keys = [], [0], [], [], [0], [], []
    for oid, rs in reach_sets.items():
        if oid not in index:
            raise ValueError(f"reach-set obstacle {oid} is not in the predictions")
        if len(rs) == 0:
            raise ValueError(f"reach-set obstacle {oid} has no parts")
        time_t = np.array([list(part.keys())[0] for part in rs])
        steps = np.array(time_t / dt - 1, dtype=int)
        for part, t, st in zip(rs, time_t, steps):
            if not t > 0:
                continue
            poly = np.asarray(list(part.values())[0], np.float64).reshape(-1, 2)
            if len(poly) < 3:
                raise ValueError(f"reach-set obstacle {oid}, time {t}: a polygon needs at least 3 vertices")
            if st < 0 or (n_steps is not None and st >= n_steps):
                raise ValueError(f"reach-set obstacle {oid}, time {t}: step index {st} outside the trajectory ({n_steps} points)")
            part_step.append(int(st))
            part_obs.append(index[oid])
            verts.append(poly)
            vert_off.append(vert_off[-1] + len(poly))
        keys.append(oid)
        entry_obs.append(index[oid])
        entry_off.append(len(part_step))
    i32 = lambda a: np.asarray(a, np.int32)
    return dict(entry_obs=i32(entry_obs), entry_part_off=i32(entry_off), part_step=i32(part_step), part_obs=i32(part_obs),
                part_vert_off=i32(vert_off), verts=np.concatenate(verts) if verts else np.zeros((0, 2)), keys=keys)


def risk_cost_params(weights, boundary_harm=None, harm_coeff=None, responsibility=None, eps: float = 10e-10,
                     scale: float = 10) -> _abi.FxRiskCostParams:
    """FxRiskCostParams.  weights: the five weights of the total, a dict by _abi.RISK_COST_NAMES (missing: 0) or a sequence in that
    order.  boundary_harm: None (0), an [n] array in the order of the evaluated candidates, or "step" with harm_coeff = (const,
    speed) of harm_parameters.json log_reg.ignore_angle -- derived on the device from the step's road-boundary stage.
    responsibility: None (the cost is 0), the [K] vector of action_space_responsibility, or "reach_set" (FrenetEngine.set_reach_sets).
    eps / scale: get_maximin_costs' defaults."""
    p = _abi.FxRiskCostParams()
    if isinstance(weights, dict):
        unknown = set(weights) - set(_abi.RISK_COST_NAMES)
        if unknown:
            raise ValueError(f"unknown risk-cost weights {sorted(unknown)}")
        weights = [weights.get(n, 0.0) for n in _abi.RISK_COST_NAMES]
    if len(weights) != 5:
        raise ValueError("five weights: " + ", ".join(_abi.RISK_COST_NAMES))
    for i, w in enumerate(weights):
        p.weights[i] = float(w)
    p.maximin_eps, p.maximin_scale = float(eps), float(scale)
    p._keep, p._lengths = [], {}   # the arrays behind the structure's pointers live as long as it does
    if boundary_harm is None:
        p.boundary_mode = _abi.FX_RISK_BOUNDARY_ZERO
    elif isinstance(boundary_harm, str):
        if boundary_harm != "step" or harm_coeff is None:
            raise ValueError('boundary_harm: None, an array, or "step" with harm_coeff=(const, speed)')
        p.boundary_mode = _abi.FX_RISK_BOUNDARY_STEP
        p.boundary_c, p.boundary_s = float(harm_coeff[0]), float(harm_coeff[1])
    else:
        a = np.ascontiguousarray(boundary_harm, dtype=np.float64).reshape(-1)
        p._keep.append(a)
        p._lengths["boundary_harm"] = len(a)
        p.boundary_mode, p.boundary_harm = _abi.FX_RISK_BOUNDARY_ARRAY, a.ctypes.data
    if responsibility is None:
        p.responsibility_mode = _abi.FX_RISK_RESP_NONE
    elif isinstance(responsibility, str):
        if responsibility != "reach_set":
            raise ValueError('responsibility: None, a [K] 0/1 vector, or "reach_set"')
        p.responsibility_mode = _abi.FX_RISK_RESP_REACH_SET
    else:
        a = np.ascontiguousarray(responsibility, dtype=np.float64).reshape(-1)
        p._keep.append(a)
        p._lengths["responsibility"] = len(a)
        p.responsibility_mode, p.responsibility = _abi.FX_RISK_RESP_ACTION_SPACE, a.ctypes.data
    return p
