"""NumPy restatement of the collision probability as the prediction cost -- test infrastructure.

get_collision_probability_fast (risk_assessment/collision_probability.py:141-261) per obstacle and ego step, and the summation
of prediction_costs (partial_cost_functions.py:344-356, its commented-out branch): np.sum per prediction, then += in dict order.
The probability part is the one of tests/risk_restatement.calc_risk (the same source lines), with that module's Genz BVNU;
vectorised over candidates: x, y, th are [C, L] (L = len(traj.cartesian.x)).
"""
import numpy as np

from tests.risk_restatement import bvnu


def step_probabilities(x, y, th, pr, ego_length, ego_width):
    """[C, L - 1]: entry i - 1 is the probability of ego point i against prediction i - 1 of `pr` (0 for i >= len(pos_list))"""
    x, y, th = (np.atleast_2d(np.asarray(a, np.float64)) for a in (x, y, th))
    C, L = x.shape
    pos = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
    covs = np.asarray(pr["cov_list"], np.float64).reshape(-1, 2, 2)
    yaw = np.asarray(pr["orientation_list"], np.float64)
    length = pr["shape"]["length"]
    off = np.array([ego_length / 6, ego_width / 2])
    prob = np.zeros((C, max(L - 1, 0)))
    for i in range(1, L):
        if i >= len(pos):
            continue
        m0 = pos[i - 1]
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
    return prob


def prediction_probability(x, y, th, predictions, ego_length, ego_width):
    """(prob [C], prob_obs [C, K], steps [C, K, L - 1]): the cost, its per-prediction sums in dict order, the probabilities"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    C, L = x.shape
    K = len(predictions)
    steps = np.zeros((C, K, max(L - 1, 0)))
    for k, pr in enumerate(predictions.values()):
        steps[:, k] = step_probabilities(x, y, th, pr, ego_length, ego_width)
    prob_obs = steps.sum(axis=2)
    prob = np.zeros(C)
    for k in range(K):
        prob = prob + prob_obs[:, k]
    return prob, prob_obs, steps


def gate_distances(x, y, pr):
    """[C, n] the three mean distances' minimum of every (candidate, step with a prediction): what the 5 m gate compares"""
    x, y = (np.atleast_2d(np.asarray(a, np.float64)) for a in (x, y))
    L = x.shape[1]
    pos = np.asarray(pr["pos_list"], np.float64).reshape(-1, 2)
    yaw = np.asarray(pr["orientation_list"], np.float64)
    out = []
    for i in range(1, min(L, len(pos))):
        dev = np.array([np.cos(yaw[i]), np.sin(yaw[i])]) * pr["shape"]["length"] / 2
        out.append(np.min([np.sqrt((mu[0] - x[:, i]) ** 2 + (mu[1] - y[:, i]) ** 2) for mu in (pos[i - 1], pos[i - 1] + dev, pos[i - 1] - dev)],
                          axis=0))
    return np.stack(out, axis=1) if out else np.zeros((x.shape[0], 0))


def near_gate(x, y, predictions, tol=1e-6):
    """[C] bool: a (step, obstacle) pair within tol of the 5 m gate"""
    near = np.zeros(np.atleast_2d(x).shape[0], bool)
    for pr in predictions.values():
        near |= np.any(np.abs(gate_distances(x, y, pr) - 5.0) <= tol, axis=1)
    return near


def resum(raw_costs, weights, n_pred, prob, deferred=False):
    """The weighted cost sum of the step's raw cost rows raw_costs [n, n_cost] with column n_pred replaced by prob, in the order
    of the device's cost sum (fx_eval_kernel.h finish_candidate): sum = -0.0, sum += w * c per term, total = 0.0 + sum; no fused
    multiply-add anywhere (NumPy multiplies and adds separately, the library is compiled with -ffp-contract=off).  deferred:
    the terms behind the prediction enter as one addend (fx_obstacle_kernel.h)."""
    raw = np.array(raw_costs, np.float64)
    raw[:, n_pred] = prob
    s = np.full(raw.shape[0], -0.0)
    tail = np.zeros(raw.shape[0])
    for m in range(raw.shape[1]):
        t = weights[m] * raw[:, m]
        if deferred and m > n_pred:
            tail = tail + t
        else:
            s = s + t
    if deferred and n_pred + 1 < raw.shape[1]:
        s = s + tail
    return 0.0 + s


def best_index(total, flags, ids=None):
    """lexicographic (total, index) minimum over SELECTABLE & ~COLLISION & ~BOUNDARY, NaN skipped; -1 when nothing is left"""
    total, flags = np.asarray(total), np.asarray(flags)
    ids = np.arange(len(total)) if ids is None else np.asarray(ids)
    pool = ((flags & 0x20) != 0) & ((flags & 0x44) == 0) & ~np.isnan(total)
    if not pool.any():
        return -1
    j = np.nonzero(pool)[0]
    order = np.lexsort((ids[j], total[j]))
    return int(ids[j[order[0]]])
