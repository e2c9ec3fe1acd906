"""NumPy restatement of the reference's calc_risk (risk_costs.py:20-118, crash_angle_simplified) -- test infrastructure.

Written from the reference's Python, independently of the product's risk.py / fx_risk_kernel.h: the harm model is chosen from
the risk.json / harm_parameters.json dicts as get_model does, the rectangle probability of mvnun by Genz's BVNU.  Vectorised
over candidates: planes x, y, theta, v are [C, L] (L = len(traj.cartesian.x)).
"""
import numpy as np
from scipy.special import ndtr, owens_t

PROTECTION = {"car": True, "truck": True, "bus": True, "bicycle": False, "pedestrian": False, "priorityvehicle": True,
              "parkedvehicle": True, "train": True, "motorcycle": False, "taxi": True, "roadboundary": None, "pillar": None,
              "constructionzone": None, "building": None, "medianstrip": None, "unknown": False}

_X = {3: [0.9324695142031522, 0.6612093864662647, 0.2386191860831970],
      6: [0.9815606342467191, 0.9041172563704750, 0.7699026741943050, 0.5873179542866171, 0.3678314989981802, 0.1252334085114692],
      10: [0.9931285991850949, 0.9639719272779138, 0.9122344282513259, 0.8391169718222188, 0.7463319064601508,
           0.6360536807265150, 0.5108670019508271, 0.3737060887154196, 0.2277858511416451, 0.07652652113349733]}
_W = {3: [0.1713244923791705, 0.3607615730481384, 0.4679139345726904],
      6: [0.04717533638651177, 0.1069393259953183, 0.1600783285433464, 0.2031674267230659, 0.2334925365383547, 0.2491470458134029],
      10: [0.01761400713915212, 0.04060142980038694, 0.06267204833410906, 0.08327674157670475, 0.1019301198172404,
           0.1181945319615184, 0.1316886384491766, 0.1420961093183821, 0.1491729864726037, 0.1527533871307259]}


def bvnu(h, k, r):
    """P(X > h, Y > k) of the standard bivariate normal with correlation r (scalar); h, k arrays (Genz 2004)."""
    h = np.asarray(h, np.float64)
    k = np.asarray(k, np.float64)
    if r == 0:
        return ndtr(-h) * ndtr(-k)
    tp = 2 * np.pi
    hk = h * k
    ar = abs(r)
    ng = 3 if ar < 0.3 else (6 if ar < 0.75 else 10)
    x = np.array(_X[ng])
    x = np.concatenate([1 - x, 1 + x])
    w = np.array(_W[ng] * 2)
    if ar < 0.925:
        hs = (h * h + k * k) / 2
        asr = np.arcsin(r) / 2
        sn = np.sin(asr * x)
        bvn = np.zeros_like(h)
        for j in range(2 * ng):
            bvn = bvn + w[j] * np.exp((sn[j] * hk - hs) / (1 - sn[j] * sn[j]))
        bvn = bvn * asr / tp + ndtr(-h) * ndtr(-k)
    else:
        if r < 0:
            k = -k
            hk = -hk
        bvn = np.zeros_like(h)
        if ar < 1:
            as_ = 1 - r * r
            a = np.sqrt(as_)
            bs = (h - k) * (h - k)
            c = (4 - hk) / 8
            d = (12 - hk) / 80
            asr = -(bs / as_ + hk) / 2
            bvn = np.where(asr > -100, a * np.exp(asr) * (1 - c * (bs - as_) * (1 - d * bs) / 3 + c * d * as_ * as_), 0.0)
            b = np.sqrt(bs)
            sp = 2.5066282746310002 * ndtr(-b / a)
            bvn = np.where(hk > -100, bvn - np.exp(-hk / 2) * sp * b * (1 - c * bs * (1 - d * bs) / 3), bvn)
            ah = a / 2
            s = np.zeros_like(h)
            for j in range(2 * ng):
                xs = (ah * x[j]) * (ah * x[j])
                asr = -(bs / xs + hk) / 2
                spj = 1 + c * xs * (1 + 5 * d * xs)
                rs = np.sqrt(1 - xs)
                ep = np.exp(-(hk / 2) * xs / ((1 + rs) * (1 + rs))) / rs
                s = s + np.where(asr > -100, np.exp(asr) * (spj - ep) * w[j], 0.0)
            bvn = (ah * s - bvn) / tp
        if r > 0:
            bvn = bvn + ndtr(-np.maximum(h, k))
        else:
            L = np.where(h < 0, ndtr(k) - ndtr(h), ndtr(-h) - ndtr(-k))
            bvn = np.where(h >= k, -bvn, L - bvn)
    return np.clip(bvn, 0.0, 1.0)


def bvn_lower_owens(h, k, r):
    """P(X < h, Y < k) through Owen's T -- an algorithm independent of Genz's (for the cross-check and the golden shim)."""
    h = np.asarray(h, np.float64)
    k = np.asarray(k, np.float64)
    h, k = np.broadcast_arrays(h, k)
    sq = np.sqrt(1 - r * r)
    out = np.empty(h.shape)
    for idx in np.ndindex(h.shape):
        a, b = float(h[idx]), float(k[idx])
        if a == 0 and b == 0:
            out[idx] = 0.25 + np.arcsin(r) / (2 * np.pi)
            continue
        if a == 0:
            a = 1e-300
        if b == 0:
            b = 1e-300
        beta = 0.0 if (a * b > 0 or (a * b == 0 and a + b >= 0)) else 0.5
        out[idx] = 0.5 * ndtr(a) + 0.5 * ndtr(b) - owens_t(a, (b - r * a) / (a * sq)) - owens_t(b, (a - r * b) / (b * sq)) - beta
    return out


def rect_probability_owens(lower, upper, mean, cov):
    """P(lower < X < upper), X ~ N(mean, cov) in two dimensions, by Owen's T (mvnun's quantity)."""
    sx, sy = np.sqrt(cov[0][0]), np.sqrt(cov[1][1])
    r = cov[1][0] / sy / sx
    a1, a2 = (lower[0] - mean[0]) / sx, (lower[1] - mean[1]) / sy
    b1, b2 = (upper[0] - mean[0]) / sx, (upper[1] - mean[1]) / sy
    F = lambda x, y: float(bvn_lower_owens(x, y, r))
    return F(b1, b2) - F(a1, b2) - F(b1, a2) + F(a1, a2)


def _bins(angle, blk, kind, sym):
    shape = np.shape(angle)
    a = np.asarray(angle, np.float64).ravel()
    out = np.empty_like(a)
    pi = np.pi
    for i, v in enumerate(a):
        if kind == "complete":
            e = [15 / 180 * pi, 45 / 180 * pi, 75 / 180 * pi, 105 / 180 * pi, 135 / 180 * pi, 165 / 180 * pi]
            names = ([("Imp_1_11", "Imp_1_11"), ("Imp_2_10", "Imp_2_10"), ("Imp_3_9", "Imp_3_9"), ("Imp_4_8", "Imp_4_8"),
                      ("Imp_5_7", "Imp_5_7")] if sym else
                     [("Imp_11", "Imp_1"), ("Imp_10", "Imp_2"), ("Imp_9", "Imp_3"), ("Imp_8", "Imp_4"), ("Imp_7", "Imp_5")])
            last = "Imp_6"
        else:
            t_a = 45 / 180 * pi
            e = [t_a, 3 * t_a] if sym else [45 / 180 * pi, 135 / 180 * pi]
            names = [("side", "side")] if sym else [("driver_side", "right_side")]
            last = "rear"
        if -e[0] < v < e[0]:
            out[i] = 0
            continue
        for j in range(1, len(e)):
            if e[j - 1] <= v < e[j]:
                out[i] = blk[names[j - 1][0]]
                break
            if -e[j - 1] >= v > -e[j]:
                out[i] = blk[names[j - 1][1]]
                break
        else:
            out[i] = blk[last]
    return out.reshape(shape)


def _models(modes, coeff, protection):
    """(ego_harm(dv, angle), obstacle_harm(dv, angle)) as get_model chooses them; raises where the reference fails."""
    if modes.get("crash_angle_simplified") is False:
        raise NotImplementedError("crash_angle_simplified: false")
    hm = modes["harm_mode"]
    if hm not in ("log_reg", "ref_speed", "gidas"):
        raise ValueError("harm_mode")
    if protection is None:
        raise ValueError("no protection class")
    ped = lambda c: (lambda v, a: 1 / (1 + np.exp(c["const"] - c["speed"] * v)))
    if hm == "gidas":
        if protection:
            raise ValueError("gidas with a protected obstacle")
        g = coeff["gidas"]
        return (lambda v, a: 1 / (1 + np.exp(-g["const"] - g["speed"] * v))), ped(coeff["pedestrian_MAIS2+"])
    if hm == "log_reg":
        ig = coeff["log_reg"]["ignore_angle"]
        lr_ig = lambda v, a: 1 / (1 + np.exp(- ig["const"] - ig["speed"] * v))
        if not protection:
            return lr_ig, ped(coeff["pedestrian"])
        if modes["ignore_angle"]:
            return lr_ig, lr_ig
        kind = "reduced" if modes["reduced_angle_areas"] else "complete"
        sym = bool(modes["sym_angle"])
        blk = coeff["log_reg"][("reduced" if kind == "reduced" else "complete") + ("_sym" if sym else "") + "_angle_areas"]
        f = lambda v, a: 1 / (1 + np.exp(- blk["const"] - blk["speed"] * v - _bins(a, blk, kind, sym)))
        return f, f
    rs = coeff["ref_speed"]["ignore_angle"]

    def rs_ig(v, a):
        temp = np.power(v / rs["ref_speed"], rs["exp"])
        return np.where(v < rs["ref_speed"], temp, 1.0)
    if not protection:
        return rs_ig, ped(coeff["pedestrian"])
    if modes["ignore_angle"]:
        return rs_ig, rs_ig
    raise ValueError("ref_speed impact-area model with a protected obstacle fails upstream")


def calc_risk(x, y, th, v, predictions, types, modes, coeff, ego_length, ego_width, ego_mass):
    """(ego_risk [C], obst_risk [C]) -- calc_risk's two scalars for each candidate row of the planes."""
    x, y, th, v = (np.atleast_2d(np.asarray(a, np.float64)) for a in (x, y, th, v))
    C, L = x.shape
    ego = np.full(C, -np.inf)
    obst = np.full(C, -np.inf)
    any_ = False
    off = np.array([ego_length / 6, ego_width / 2])
    for oid, pr in predictions.items():
        key = str(types[oid]).replace("_", "").lower()
        prot = PROTECTION[key]
        ego_f, obs_f = _models(modes, coeff, prot)
        pos = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
        covs = np.asarray(pr["cov_list"], np.float64).reshape(-1, 2, 2)
        yaw = np.asarray(pr["orientation_list"], np.float64)
        vo = np.asarray(pr["v_list"], np.float64)
        length, width = pr["shape"]["length"], pr["shape"]["width"]
        pl = min(L - 1, len(pos))
        if pl == 0:
            continue
        # collision probability [C, L-1]
        prob = np.zeros((C, L - 1))
        inv = np.linalg.inv(covs) if modes.get("fast_prob_mahalanobis") else None
        for i in range(1, L):
            if i >= len(pos):
                continue
            m0 = pos[i - 1]
            if inv is not None:
                d0, d1 = x[:, i] - m0[0], y[:, i] - m0[1]
                iv = inv[i - 1]
                r0, r1 = d0 * iv[0, 0] + d1 * iv[1, 0], d0 * iv[0, 1] + d1 * iv[1, 1]
                m = r0 * d0 + r1 * d1
                prob[:, i - 1] = 1.0 / (m ** 2)
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
                    p = p + (((bvnu(a1, a2, r) - bvnu(b1, a2, r)) - bvnu(a1, b2, r)) + bvnu(b1, b2, r))
            prob[live, i - 1] = p / 3
        # harm [C, pl]
        mass_o = _mass(key, length * width)
        pdof = yaw[:pl] - th[:, :pl] + np.pi
        rel = np.arctan2(pos[:pl, 1] - y[:, :pl], pos[:pl, 0] - x[:, :pl])
        ego_angle = rel - th[:, :pl]
        obs_angle = np.pi + rel - yaw[:pl]
        dv = np.sqrt(v[:, :pl] ** 2 + vo[:pl] ** 2 + 2 * v[:, :pl] * vo[:pl] * np.cos(pdof))
        he = np.broadcast_to(ego_f(mass_o / (ego_mass + mass_o) * dv, ego_angle.copy()), (C, pl))
        ho = np.broadcast_to(obs_f(ego_mass / (ego_mass + mass_o) * dv, obs_angle.copy()), (C, pl))
        ego = np.maximum(ego, (he * prob[:, :pl]).max(axis=1))
        obst = np.maximum(obst, (ho * prob[:, :pl]).max(axis=1))
        any_ = True
    if not any_:
        return np.zeros(C), np.zeros(C)
    return ego, obst


def _mass(key, size):
    if key in ("car", "priorityvehicle", "parkedvehicle", "taxi"):
        return -1333.5 + 526.9 * np.power(size, 0.8)
    return {"truck": 25000, "bus": 13000, "bicycle": 90, "pedestrian": 75, "train": 118800, "motorcycle": 250}.get(key, 0)


def min_risk_index(ego, obst, ids):
    """sorted(feasible, key=ego + obst)[0] over candidates `ids` in creation order"""
    s = np.asarray(ego) + np.asarray(obst)
    return int(ids[int(np.argmin(s))]) if len(ids) else -1
