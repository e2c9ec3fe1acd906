"""fx_select_kernel at the candidate counts where it changes its path, on scenes built to have cost ties around the winner.

The winner comes from partials the evaluation kernel writes, so these are real steps.  The slice count of the selection
(fx_launch_select) is 32 up to 131 072 candidates, 64 up to 262 144, 128 above; a workgroup pre-loads 8 x 256 (flag, cost) pairs
and runs a second loop only when its slice holds more, i.e. above 65 536 candidates at 32 slices
(tests/test_topk_planes.py::test_switch_sizes_follow_the_source holds these sizes to the source).

Scene: a straight reference, 3 s horizon, end times 1.1 ... 1.5 s, `velocity_offset` alone as the cost -- it reads the speed
from 1.5 s on, where every candidate of an end velocity drives that velocity, so the candidates of one end velocity share one
cost whatever their end time and offset: 151 ... 726 distinct costs among 26 000 ... 105 000 selectable candidates.  Six obstacles, a slow
lead vehicle 20 m ahead: 94 % of the selectable candidates collide.  The grid is handed over as a sampling matrix whose rows are
a seeded permutation of the grid's, cut to the candidate count: the tied and the colliding candidates lie all over the index
range, and the permutation's seed was searched on the CPU oracle until every precondition below holds (at 65 537, 131 073 and
262 145 candidates a slice holds 2 049: ONE candidate per slice lies behind the pre-load).

Compared: (best_index, best_cost, n_collisions) of the step with NumPy on the device's own costs() -- the lexsort minimum of
the eligible candidates, the SELECTABLE & COLLISION candidates ordered before it (csrc/fx_select.h, head comment) -- exactly, and
with oracle.plan_step on the same inputs."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import synthetic
from tests import device_planes as dp

FRAGILE = 1e-9
# candidate count -> seed of the row permutation
PERMUTATION = {65_536: 0, 65_537: 50, 131_072: 0, 131_073: 53, 262_145: 6}
assert tuple(PERMUTATION) == dp.SELECT_SIZES


def scene(C: int, hull_builder, *, v0: float = 25.0):
    """5 end times x ceil(C / 500) end velocities x 100 offsets, rows permuted, the first C"""
    kw = dict(ref_kind="straight", v0=v0, v_des=v0 + 1.0, grid=(5, -(-C // 500), 99), n_obstacles=6, n_pred=30, horizon=3.0, seed=2,
              lead_gap=20.0, cost_weights={"velocity_offset": 1.0}, write_bundle=False, write_costmap=False, as_matrix=True)
    inp = synthetic.make_inputs(hull_builder=hull_builder, **kw)
    n = inp.n_candidates
    assert n >= C and n - C < 500
    rows = np.random.default_rng([C, PERMUTATION[C]]).permutation(n)[:C]
    inp.sampling_matrix = np.ascontiguousarray(inp.sampling_matrix[rows])
    assert inp.n_candidates == C and inp.collision and not inp.write_bundle
    return inp


def small_scene(a: int, hull_builder):
    """an agent of a few hundred candidates for the batch"""
    return synthetic.make_inputs(hull_builder=hull_builder, ref_kind="arc", v0=6.0 + 0.25 * a, grid=(3, 9 + a % 4, 10), n_obstacles=6,
                                 lead_gap=10.0 + a % 5, seed=100 + a, cost_weights={"velocity_offset": 1.0}, write_bundle=False, write_costmap=False)


def preconditions(C: int, cost, flags, n_slices: int):
    """What makes the scene a test of the tie rule and of the second loop; asserted on the oracle's planes and on the device's."""
    w, wc, count, counted = dp.expected_selection(cost, flags)
    assert w >= 0 and count > 0, (w, count)
    colliding = np.nonzero(((flags & dp.SEL) != 0) & ((flags & dp.COL) != 0))[0]
    tied = colliding[cost[colliding] == wc]
    assert (tied < w).any() and (tied > w).any(), "no colliding candidate of the winner's cost on both sides of it"
    if C > dp.SELECT_SLICES_MIN * dp.SELECT_PRELOAD:
        off = dp.select_slice_offset(C, n_slices, counted)
        assert (off >= dp.SELECT_PRELOAD).any(), "no counted candidate behind the pre-loaded pairs of its slice"
        assert ((off >= dp.SELECT_PRELOAD) & (off < dp.SELECT_PRELOAD + 256)).any(), "none in the second loop's first 256"
        # a tied colliding candidate BEHIND the winner there: counted by a second loop that forgets the index rule
        assert (dp.select_slice_offset(C, n_slices, tied[tied > w]) >= dp.SELECT_PRELOAD).any()
    return w, wc, count


def triple(res):
    return res["best_index"], res["best_cost"], res["n_collisions"]


def hold_to_own_planes(res, cost, flags):
    w, wc, count, _ = dp.expected_selection(cost, flags)
    assert res["best_index"] == w and res["n_collisions"] == count, (triple(res), (w, wc, count))
    if w >= 0:
        assert int(dp.bits(res["best_cost"])) == int(dp.bits(wc))


def hold_to_oracle(res, out, flags):
    """flag words and count exact; the winner exact, or -- a last-ulp cost tie, as
    test_hip_parity.py::test_winner_decided_by_a_last_ulp_cost_tie_is_an_admissible_outcome admits it -- a candidate whose
    ORACLE cost lies within 8 ulp of the oracle's winner's (the count is then held by the device's own planes alone)"""
    assert np.all(out["margin"] >= FRAGILE)
    assert np.array_equal(flags, out["flags"])
    ga, gb = res["best_index"], out["result"]["best_index"]
    if gb < 0 or ga == gb:
        assert ga == gb and res["n_collisions"] == out["result"]["n_collisions"]
        if gb >= 0:
            assert abs(res["best_cost"] - out["result"]["best_cost"]) <= 1e-9 * abs(out["result"]["best_cost"])
    else:
        assert ga >= 0 and abs(out["cost"][ga] - out["cost"][gb]) <= 8 * np.spacing(abs(out["cost"][gb]))


def test_scenes_hold_their_preconditions_on_the_oracle():
    """(no GPU) the scenes as they were fixed: a winner, collisions in front of it, ties on both sides, counted candidates behind
    the pre-load -- and no decision of any candidate taken by the last ulp, so the device owes the oracle's flag words exactly"""
    from oracle import oracle
    for C in dp.SELECT_SIZES:
        out = oracle.plan_step(scene(C, oracle.build_obstacle_hulls), want_planes=False)
        assert np.all(out["margin"] >= FRAGILE)
        w, wc, count = preconditions(C, out["cost"], out["flags"], dp.select_slices(C))
        assert (w, count) == (out["result"]["best_index"], out["result"]["n_collisions"]) and wc == out["result"]["best_cost"]
        sel = out["selectable"]
        assert len(np.unique(out["cost"][sel])) <= 2 * -(-C // 500) and sel.sum() > 20_000 and (sel & out["collision"]).sum() > 0.9 * sel.sum()
    out = oracle.plan_step(scene(131_073, oracle.build_obstacle_hulls), want_planes=False)
    preconditions(131_073, out["cost"], out["flags"], 32)            # as the batch slices it
    small = [oracle.plan_step(small_scene(a, oracle.build_obstacle_hulls), want_planes=False) for a in range(32)]
    assert sum(o["result"]["best_index"] >= 0 for o in small) > 16 and sum(o["result"]["n_collisions"] > 0 for o in small) > 16


@pytest.fixture(scope="module")
def hulls():
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return build_obstacle_hulls


@pytest.mark.gpu
@pytest.mark.parametrize("C", dp.SELECT_SIZES)
def test_selection_at_its_size_switches(C, hulls):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    out = oracle.plan_step(scene(C, oracle.build_obstacle_hulls), want_planes=False)
    n_slices = dp.select_slices(C)
    preconditions(C, out["cost"], out["flags"], n_slices)
    inp = scene(C, hulls)
    got = {}
    for leg in ("default", 0, 2):
        with FrenetEngine(max_candidates=C + 64, max_steps=inp.N) as e:
            if leg != "default":
                e.set_fused_selection(leg)
            res = e.plan_step(inp)
            info = e.step_info()
            cost, flags = e.costs()
        if leg in ("default", 0):
            assert not info["fused_selection"] and not info["step_kernel"], info   # fx_select_kernel ended the step
        print(f"C={C} leg={leg} slices={n_slices} fused={info['fused_selection']} {triple(res)}")
        preconditions(C, cost, flags, n_slices)
        hold_to_own_planes(res, cost, flags)
        hold_to_oracle(res, out, flags)
        got[leg] = triple(res)
    assert got["default"] == got[0] == got[2], got


@pytest.mark.gpu
def test_no_winner_counts_every_colliding_selectable_candidate(hulls):
    """At 40 m/s every selectable candidate of the scene runs into the lead vehicle: index -1, and the count is all of them."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    C = 65_537
    out = oracle.plan_step(scene(C, oracle.build_obstacle_hulls, v0=40.0), want_planes=False)
    assert out["result"]["best_index"] == -1 and out["selectable"].sum() > 10_000 and np.array_equal(out["selectable"], out["selectable"] & out["collision"])
    inp = scene(C, hulls, v0=40.0)
    got = {}
    for leg in ("default", 0, 2):
        with FrenetEngine(max_candidates=C + 64, max_steps=inp.N) as e:
            if leg != "default":
                e.set_fused_selection(leg)
            res = e.plan_step(inp)
            cost, flags = e.costs()
        hold_to_own_planes(res, cost, flags)
        hold_to_oracle(res, out, flags)
        assert res["best_index"] == -1 and res["n_collisions"] == int(out["selectable"].sum())
        got[leg] = (res["best_index"], res["n_collisions"])
    assert got["default"] == got[0] == got[2]


@pytest.mark.gpu
def test_batch_halves_the_slices_and_keeps_every_agents_answer(hulls):
    """33 agents, one of 131 073 candidates and 32 of a few hundred: alone the large agent is reduced in 64 slices, in the batch
    64 x 33 > 2 048 workgroups halve them to 32 (4 097 candidates per slice: the second loop) -- every agent's
    (best_index, best_cost, n_collisions) equals what the agent answers alone (64 slices for the large one)."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from tests.test_frame_invariance_gpu import _pin_decomposition
    C, n_small = 131_073, 32
    assert dp.select_slices(C, 1) == 64 and dp.select_slices(C, 1 + n_small) == 32 and dp.select_slices(C, n_small) == 64
    inps = [small_scene(a, hulls) for a in range(n_small)]
    inps.insert(7, scene(C, hulls))
    assert all(200 <= i.n_candidates <= 600 for i in inps if i.n_candidates != C)
    cap = sum(i.n_candidates + 64 for i in inps)
    with FrenetEngine(max_candidates=cap, max_steps=inps[7].N, max_agents=len(inps)) as e:
        batch = e.plan_batch(inps)
        info = e.step_info()
        assert info["agents"] == 33 and not info["fused_selection"] and not info["step_kernel"], info
        planes = [e.costs(a) for a in range(len(inps))]
        for a, res in enumerate(batch):
            hold_to_own_planes(res, *planes[a])
        preconditions(C, *planes[7], 32)
        # alone, under the batch's work decomposition (the sums of a cost follow the lanes per candidate: the automatic choice for
        # a small agent alone may differ from the batch's in the last bit of a cost)
        _pin_decomposition(e, info)
        alone = []
        for a, inp in enumerate(inps):
            alone.append(e.plan_step(inp))
            one = e.step_info()
            assert one["agents"] == 1 and all(one[k] == info[k] for k in ("lanes_per_candidate", "grid_kernel")), (one, info)
            cost, flags = e.costs()
            assert np.array_equal(dp.bits(cost), dp.bits(planes[a][0])) and np.array_equal(flags, planes[a][1]), a
    assert [triple(r) for r in batch] == [triple(r) for r in alone]
    assert sum(r["best_index"] >= 0 for r in batch) > 16 and sum(r["n_collisions"] > 0 for r in batch) > 16
