"""The list kernel on split lanes (fx_set_materialise_lanes).

At G = 8 or 32 lanes per candidate the list kernel is the generic evaluation kernel's decomposition at G lanes with the index read
from a list: the same functions, the same chunks, the same carry-in step, the same shuffle combine.  So the requirement against the
bundle the generic kernel stores when it is forced to G lanes (set_tuning(G, 0, 1)) is equality, bit for bit, of every part --
planes on the stored mask, coefficients, horizon lengths, raw costs, costs, flag words, boundary steps -- and against the select-only
step it follows (automatic tuning: another kernel, whose cost sums associate differently) equal flag words and rtol = 1e-12 on the
cost, the figure test_materialise_gpu.py holds between kernels."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests.test_materialise_gpu import BITWISE_KW, FORMS, SMALL_KW, assert_rows_equal, bundle_twin, id_lists, select_only

pytestmark = pytest.mark.gpu

LANES = (8, 32)
# a reference of 34.5 m with the ego at 20 m of it: at 12 m/s every candidate leaves the projection domain around step 12 of 31
LEAVE_KW = dict(ref_kind="arc", n_knots=70, s_knot=40, v0=12.0, grid=(5, 9, 11), n_obstacles=4, draw_traj_set=True, kinematic_debug=True)
SCENES = dict({k: FORMS[k] for k in ("matrix", "low_velocity", "horizon5", "no_obstacles", "road_boundary")},
              small=SMALL_KW, stop_point=dict(BITWISE_KW, grid=(5, 9, 11), stop_point_s=28.0), leaves_domain=LEAVE_KW)


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=120_000, max_steps=60, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64, max_agents=8)
    yield e
    e.set_materialise_lanes(1)
    e.close()


def lane_lists(C_, G):
    """one id; two out of order; the last candidate of a workgroup of 256 / G candidates, exactly one workgroup, and a second
    workgroup with one live candidate; the ragged list of 70 with duplicates; every candidate"""
    cpb = 256 // G
    rng = np.random.default_rng(23 + G)
    edge = [rng.choice(C_, size=min(n, C_), replace=False) for n in (cpb - 1, cpb, cpb + 1)]
    base = id_lists(C_)
    return [base[0], base[1]] + edge + [base[2], base[4]]


@pytest.mark.parametrize("G", LANES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_split_kernel_equals_the_generic_kernel_at_the_same_lanes(eng, name, G):
    kw = SCENES[name]
    inp_b, _, want = bundle_twin(eng, kw, tuning=(G, 0, 1))
    inp = select_only(kw)
    assert inp.n_samples == (51 if name == "horizon5" else 31)   # (G = 32: part 31 without a step; two steps per part, six parts empty)
    eng.plan_step(inp)
    cost, flags = eng.costs()
    boundary = name == "road_boundary"
    if boundary:
        assert (want["boundary_step"] >= 0).any()
    if name == "leaves_domain":
        # a listed candidate leaves the projection domain mid-horizon: reason 9 in its flag word, (x, y) zeroed behind the step
        left = ((want["flags"] >> _abi.FX_REASON_SHIFT) >> 9) & 1
        x = want["planes"][:, _abi.PLANE_NAMES.index("x"), :]
        mid = (left == 1) & (x[:, 1] != 0.0) & (x[:, inp.n_samples // 2 + 4] == 0.0)
        assert mid.any()
    eng.set_materialise_lanes(G)
    try:
        for ids in lane_lists(inp.n_candidates, G):
            got = eng.materialise(ids)
            info = eng.last_materialise_info
            assert info == dict(lanes=G, launches=1, rows=1), info
            assert_rows_equal(got, want, ids, inp_b, boundary)
            assert np.array_equal(got["flags"], flags[ids]) and np.allclose(got["cost"], cost[ids], rtol=1e-12, atol=0)
        if name == "leaves_domain":
            assert (((got["flags"] >> _abi.FX_REASON_SHIFT) >> 9) & 1).any()
    finally:
        eng.set_materialise_lanes(1)


def test_windowed_costs_run_at_one_lane(eng):
    kw = FORMS["windowed_costs"]
    inp_b, _, want = bundle_twin(eng, kw)   # the generic kernel at ONE lane
    eng.plan_step(select_only(kw))
    eng.set_materialise_lanes(8)
    try:
        for ids in id_lists(inp_b.n_candidates)[1:]:
            got = eng.materialise(ids)
            assert eng.last_materialise_info["lanes"] == 1
            assert_rows_equal(got, want, ids, inp_b)
    finally:
        eng.set_materialise_lanes(1)


def test_other_lane_counts_are_refused_and_the_setting_stays(eng):
    kw = SMALL_KW
    eng.plan_step(select_only(kw))
    eng.set_materialise_lanes(8)
    try:
        for bad in (2, 4, 16, 64, -1):
            with pytest.raises(ValueError):
                eng.set_materialise_lanes(bad)
            eng.materialise([3, 1])
            assert eng.last_materialise_info["lanes"] == 8, bad
        eng.set_materialise_lanes(0)   # 0 is one lane, as 1
        eng.materialise([3, 1])
        assert eng.last_materialise_info == dict(lanes=1, launches=1, rows=1)
    finally:
        eng.set_materialise_lanes(1)


@pytest.mark.parametrize("G", LANES)
def test_the_step_is_untouched_behind_a_split_lane_call(eng, G):
    inp = select_only(BITWISE_KW)
    res = eng.plan_step(inp)
    before = (eng.costs(), eng.topk(32), eng.step_info())
    eng.set_materialise_lanes(G)
    try:
        eng.materialise(id_lists(inp.n_candidates)[2])
        eng.materialise(np.arange(inp.n_candidates))
    finally:
        eng.set_materialise_lanes(1)
    after = (eng.costs(), eng.topk(32), eng.step_info())
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)
    assert before[2] == after[2]
    assert eng.finish()[0] == res   # the published result block: counters, histogram, winner


def test_a_planner_on_split_lanes_plans_what_the_one_lane_planner_plans():
    from tests.test_hip_planner import make_planner
    from tests.test_materialise_gpu import _pair_columns
    a, _ = make_planner(sparse_bundle_k=8)
    b, _ = make_planner(sparse_bundle_k=8, sparse_lanes=32)
    try:
        pa, pb = a.plan(), b.plan()
        assert pa is not None and pb is not None
        assert b.engine.last_materialise_info["lanes"] == 32 and a.engine.last_materialise_info["lanes"] == 1
        assert b.last_step.result["best_index"] == a.last_step.result["best_index"]
        assert b.optimal_trajectory.uniqueId == a.optimal_trajectory.uniqueId
        for ca, cb in zip(_pair_columns(pa), _pair_columns(pb)):
            assert np.allclose(cb, ca, rtol=1e-12, atol=0)
    finally:
        a.close()
        b.close()
