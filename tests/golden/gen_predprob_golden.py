"""Generate tests/golden/predprob_*.npz: the reference's own `get_collision_probability_fast`
(risk_assessment/collision_probability.py:141-261) and the summation of `prediction_costs` (partial_cost_functions.py:344-356,
the branch that sums it) on the trajectories of risk_obs5, risk_mixed_obs6 and risk_config3_obs20 -- the same planes, plane_ids
and predictions as those files (gen_risk_golden.py wrote them).

Run from the repository root with the reference tree present:  python tests/golden/gen_predprob_golden.py

The shims are gen_risk_golden's (ObstacleType, RectOBB, mvnun through Owen's T: see that file).  Per file: prob [n] the cost of
every stored trajectory, prob_obs [n, K] the np.sum per prediction, steps [n, K, L - 1] the probabilities; ego = (length, width).

Conditions asserted, so that a regenerated file cannot lose its meaning unnoticed: no trajectory has a (step, obstacle) pair
within 1e-6 m of the 5 m gate (there the reference's own decision is a matter of the last bit); exactly PASS_GATE trajectories
of the file pass the gate somewhere (9 of 90, 17 of 85, 82 of 82); and exactly POSITIVE of them have a positive sum: 5, 15 and 82.
The request behind these files was "at least as many positive sums as trajectories that pass the gate".  With the mvnun shim that
cannot hold for two files: behind the gate most sums are below 1e-15, and the shim's Owen's-T differences carry a cancellation
noise of ~1e-16, so that the reference's sums there come out as 0 or slightly negative (the restatement's Genz sums are positive
for all 9 and 17: tests/test_predprob_restatement.py).  What is asserted is what the reference gives, as exact counts, and that
every sum that is not positive is within that noise (|sum| <= 1e-15).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import gen_risk_golden as grg  # noqa: E402
from tests import predprob_restatement as pp  # noqa: E402

FILES = {"risk_obs5": "predprob_obs5", "risk_mixed_obs6": "predprob_mixed_obs6", "risk_config3_obs20": "predprob_config3_obs20"}
PASS_GATE = {"predprob_obs5": 9, "predprob_mixed_obs6": 17, "predprob_config3_obs20": 82}
POSITIVE = {"predprob_obs5": 5, "predprob_mixed_obs6": 15, "predprob_config3_obs20": 82}


def main():
    grg.install_shims()
    from risk_assessment.collision_probability import get_collision_probability_fast
    for src, name in FILES.items():
        g = np.load(os.path.join(HERE, src + ".npz"))
        keys = [int(k) for k in g["pred_keys"]]
        preds = {k: dict(pos_list=g["pred_pos"][j], cov_list=g["pred_cov"][j], orientation_list=g["pred_yaw"][j], v_list=g["pred_v"][j],
                         shape=dict(length=float(g["pred_shape"][j][0]), width=float(g["pred_shape"][j][1]))) for j, k in enumerate(keys)}
        planes = g["planes"]   # [n, 4, L]: x, y, theta, v
        n, _, L = planes.shape
        veh = types.SimpleNamespace(length=float(g["ego"][0]), width=float(g["ego"][1]))
        prob, prob_obs, steps = np.zeros(n), np.zeros((n, len(keys))), np.zeros((n, len(keys), L - 1))
        for c in range(n):
            traj = types.SimpleNamespace(cartesian=types.SimpleNamespace(x=planes[c, 0], y=planes[c, 1], theta=planes[c, 2]))
            raw = get_collision_probability_fast(traj=traj, predictions=preds, vehicle_params=veh)
            pred_costs = 0
            for j, key in enumerate(raw):   # prediction_costs: pred_costs += np.sum(raw[key])
                assert key == keys[j]
                steps[c, j] = raw[key]
                prob_obs[c, j] = np.sum(raw[key])
                pred_costs += np.sum(raw[key])
            prob[c] = pred_costs
        near = pp.near_gate(planes[:, 0], planes[:, 1], preds)
        passes = np.zeros(n, bool)
        for pr in preds.values():
            passes |= np.any(~(pp.gate_distances(planes[:, 0], planes[:, 1], pr) > 5.0), axis=1)
        assert not near.any(), f"{name}: {int(near.sum())} trajectories within 1e-6 m of the gate"
        assert int(passes.sum()) == PASS_GATE[name], (name, int(passes.sum()))
        assert int((prob > 0).sum()) == POSITIVE[name] and not (prob > 0)[~passes].any(), (name, int((prob > 0).sum()))
        assert np.all(np.abs(prob[~(prob > 0)]) <= 1e-15), (name, np.abs(prob[~(prob > 0)]).max())
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, plane_ids=g["plane_ids"], prob=prob, prob_obs=prob_obs, steps=steps, ego=g["ego"][:2],
                            n_pass_gate=np.int64(passes.sum()))
        print(f"{path}: {n} trajectories, {int(passes.sum())} pass the gate somewhere, {int((prob > 0).sum())} with a positive sum, "
              f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
