"""ReactivePlannerHip.what_if on the planner's 630-candidate step with five predicted obstacles: the last step
under other predictions dicts, packed with the planner's own packer."""
import copy

import numpy as np
import pytest

from tests import device_planes as dp

pytestmark = pytest.mark.gpu


def test_the_planner_asking_what_if():
    from tests.test_hip_planner import make_planner
    rp, _ = make_planner()
    try:
        with pytest.raises(ValueError, match="no plan step"):
            rp.what_if([rp.predictions])
        assert rp.plan() is not None
        step = rp.last_step
        assert step.inputs.n_candidates == 630 and step.inputs.obstacles["K"] == 5
        w = step.result["best_index"] - step.inputs.shard_begin
        # the step's own predictions name last_step's device winner; an empty world has no collision and no prediction cost
        keys = list(rp.predictions)
        fewer = {k: rp.predictions[k] for k in keys[:2]}
        onto = copy.deepcopy(rp.predictions)
        x, y, th = (step.engine.plane(n, step.agent)[:, w] for n in ("x", "y", "theta"))
        onto[keys[0]] = dict(onto[keys[0]], pos_list=np.stack([x[1:], y[1:]], axis=1), orientation_list=np.array(th[1:]))
        out = rp.what_if([rp.predictions, {}, fewer, onto])
        assert len(out) == 4 and all(len(o) == 3 for o in out)
        assert out[0][0] == w and out[0][2] == step.result["n_collisions"]
        # (a planner-sized step runs its obstacle stage inside the walk: the cost agrees within the suite's 1e-9 door, the bits are
        # those of the split form -- tests/test_hypotheses_steps_gpu.py)
        assert abs(out[0][1] - step.result["best_cost"]) <= 1e-9 * abs(step.result["best_cost"])
        assert out[1][2] == 0 and out[1][0] >= 0 and out[1][1] <= out[0][1]
        assert out[3][0] != w                       # an obstacle on the winner's path: another winner
        with pytest.raises(ValueError, match="obstacles in a hypothesis"):
            rp.what_if([dict(rp.predictions, extra=rp.predictions[keys[0]])])
        # nothing of the planner moved
        assert rp.last_step is step and step.result["best_index"] - step.inputs.shard_begin == w
    finally:
        rp.close()
