"""The device sort behind real plan steps: PlanStepResult.ranked_ids against the host's sorted_ids() on
synthetic scenes with obstacles, the planner's walk by rank, and a rank range fed to materialise()."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, synthetic
from frenetix_motion_planner_amd.trajectories import PlanStepResult
from tests import device_planes as dp
from tests import sort_planes as sp
from tests.test_hip_parity import hip_hulls
from tests.test_materialise_gpu import BITWISE_KW

pytestmark = pytest.mark.gpu

# 7 x 9 x 34 = 2 142 candidates: the one-workgroup kernel; 7 x 17 x 48 = 5 712: three tiles, the last ragged
SCENES = {"one_workgroup": BITWISE_KW, "tiled": dict(BITWISE_KW, grid=(7, 17, 47))}


@pytest.fixture(autouse=True)
def sort_any_size(monkeypatch):
    """the scenes here are a few thousand candidates, below the measured size from which ranked_ids sorts on the device
    (trajectories.DEVICE_SORT_MIN_CANDIDATES): these tests are about the device's order, so it sorts whatever the size"""
    from frenetix_motion_planner_amd import trajectories
    monkeypatch.setattr(trajectories, "DEVICE_SORT_MIN_CANDIDATES", 0)


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=120_000, max_steps=60, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64)
    yield e
    e.close()


@pytest.mark.parametrize("bundle", (True, False))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_ranked_ids_equal_the_host_order(eng, scene, bundle):
    """a bundle step and a select-only step: the whole pool by rank equals sorted_ids(), for COSTED and for SELECTABLE"""
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), write_bundle=bundle, write_costmap=bundle, **SCENES[scene])
    assert (inp.n_candidates > sp.SORT_SMALL_MAX) == (scene == "tiled") and inp.n_candidates % 64 != 0
    res = eng.plan_step(inp)
    step = PlanStepResult(eng, inp, res)
    got = {}
    for bit in (_abi.FX_FLAG_COSTED, _abi.FX_FLAG_SELECTABLE):
        n_pool, n_nan = step.ranked_count(bit)
        got[bit] = (n_pool, n_nan, step.ranked_ids(0, n_pool, bit), step.ranked_ids(64, 32, bit), step.ranked_ids(n_pool - 5, 50, bit))
    assert step._cost is None                                   # nothing above read the C costs
    for bit, (n_pool, n_nan, ids, page, tail) in got.items():
        want = step.sorted_ids(bit)
        assert n_pool == len(want) > 200 and n_nan == int(np.isnan(step.cost[want]).sum())
        assert np.array_equal(ids, want) and np.array_equal(page, want[64:96]) and np.array_equal(tail, want[-5:])
    assert res["n_collisions"] > 0 or (step.flags & _abi.FX_FLAG_COLLISION).any()      # (the scene has obstacles in the way)
    # the survivor pool's first ranks are the top-k
    n_pool, n_nan = step.ranked_count(sp.SEL, sp.COL | sp.BND)
    _, idx = eng.topk(64)
    k = min(64, n_pool - n_nan)
    assert k > 16 and np.array_equal(step.ranked_ids(0, k, sp.SEL, sp.COL | sp.BND), idx[0][:k])


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_a_rank_range_feeds_materialise(eng, scene):
    """materialise(ranked_ids(64, 32)) of a select-only step: the rows of ranks 64 ... 95, in that order"""
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), write_bundle=False, write_costmap=False, **SCENES[scene])
    res = eng.plan_step(inp)
    step = PlanStepResult(eng, inp, res)
    ids = step.ranked_ids(64, 32)
    assert len(ids) == 32
    rows = eng.materialise(ids)
    cost, flags = eng.costs()
    assert np.array_equal(rows["flags"], flags[ids]) and np.allclose(rows["cost"], cost[ids], rtol=1e-12, atol=0)
    assert np.all(np.diff(cost[ids]) >= 0) and rows["planes"].shape[0] == 32 and np.isfinite(rows["planes"][:, 0]).all()
    # an existing materialised set is what it was after another sort
    before = eng.materialised_package(int(ids[3]))
    assert eng.sort_candidates(0, sp.SEL, sp.COL | sp.BND)[0] > 0 and len(eng.ranked(0, 8)) == 8
    after = eng.materialised_package(int(ids[3]))
    assert np.array_equal(dp.bits(before.block), dp.bits(after.block)) and before.cost == after.cost and before.index == after.index
    again = eng.materialise(ids)
    assert all(np.array_equal(rows[k], again[k]) for k in ("planes", "lon", "lat", "cost", "flags", "raw_costs"))


def test_below_the_switch_size_the_host_arrays_answer(eng, monkeypatch):
    """the default switch: a step of 2 142 candidates is ordered from its host arrays, the same ids, and nothing is sorted"""
    from frenetix_motion_planner_amd import trajectories
    monkeypatch.undo()
    assert trajectories.DEVICE_SORT_MIN_CANDIDATES == 13_000
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **SCENES["one_workgroup"])
    step = PlanStepResult(eng, inp, eng.plan_step(inp))
    serial = eng.sort_serials.get(0, 0)
    ids = step.ranked_ids(64, 32)
    assert step._cost is not None and eng.sort_serials.get(0, 0) == serial and np.array_equal(ids, step.sorted_ids()[64:96])
    monkeypatch.setattr(trajectories, "DEVICE_SORT_MIN_CANDIDATES", 0)
    assert np.array_equal(step.ranked_ids(64, 32), ids) and eng.sort_serials[0] == serial + 1


def _planner(**cfg):
    from tests.test_hip_planner import make_planner
    return make_planner(**cfg)[0]


def _plan_with_rejections(n_reject, **cfg):
    rp = _planner(**cfg)
    seen = []

    def check(traj):
        seen.append(traj.uniqueId)
        return 0.7 if len(seen) <= n_reject else 0

    rp.road_boundary_check = check
    pair = rp.plan()
    step = rp.last_step
    order = step._host_order(sp.SEL, sp.COL | sp.BND)
    order = order[~np.isnan(step.cost[order])]
    chosen = None if rp.optimal_trajectory is None else rp.optimal_trajectory.uniqueId
    n_all = len(rp.all_traj) if rp.all_traj is not None else None
    first = [t.uniqueId for t in rp.all_traj[:40]]
    rp.close()
    return pair, chosen, seen, order, n_all, first


@pytest.mark.parametrize("sparse", (0, 8))
def test_planner_by_rank(sparse):
    """device_sort=True: the identical trajectory where the default finds one; the 17th-plus survivor where a rejecting
    road_boundary_check makes the default fall back -- on a step that stores everything and on a select-only one"""
    for n_reject in (0, 3):
        a = _plan_with_rejections(n_reject, sparse_bundle_k=sparse)
        b = _plan_with_rejections(n_reject, sparse_bundle_k=sparse, device_sort=True)
        assert a[0] is not None and b[0] is not None and a[1] == b[1] == a[3][n_reject] and a[2] == b[2]
        assert a[4] == b[4] and a[5] == b[5]                     # all_traj: the same length and the same first page
    for n_reject in (16, 70):
        a = _plan_with_rejections(n_reject, sparse_bundle_k=sparse)
        b = _plan_with_rejections(n_reject, sparse_bundle_k=sparse, device_sort=True)
        assert len(a[3]) > n_reject + 1
        assert a[0] is None and a[1] is None and a[2] == a[3][:16].tolist()               # today: the fallback
        assert b[0] is not None and b[1] == b[3][n_reject] and b[2] == b[3][:n_reject + 1].tolist()


def test_sparse_bundle_beyond_the_topk_bound():
    """sparse_bundle_k = 100 with device_sort: the winner and the first 100 survivors are materialised"""
    rp = _planner(sparse_bundle_k=100, device_sort=True)
    assert rp.plan() is not None
    step = rp.last_step
    order = step._host_order(sp.SEL, sp.COL | sp.BND)
    assert len(order) > 100 and set(order[:100].tolist()) <= set(step._mat_ids.tolist()) and len(step._mat_ids) <= 101
    assert np.isfinite(step.sample(int(order[99])).cartesian.x).all()
    rp.close()


def test_handler_switch():
    """frenetix_compat.TrajectoryHandler.device_sort: get_sorted_trajectories() by rank is the host's list"""
    from tests.handler_fixture import evaluate, make_handler
    got = []
    for device_sort in (False, True):
        h, matrix = make_handler()
        h.device_sort = device_sort
        h.reset_Trajectories()
        evaluate(h, matrix())
        trajs = h.get_sorted_trajectories()
        got.append([t.uniqueId for t in trajs])
        costs = [t.cost for t in trajs]
        assert costs == sorted(costs)
        h.engine.close()
    assert len(got[0]) == 800 and got[0] == got[1]
