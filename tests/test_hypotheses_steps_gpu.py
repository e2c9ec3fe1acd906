"""The hypotheses pass (FrenetEngine.hypotheses, fx_eval_hypotheses_agent) behind real plan steps.

Two engines: the first runs the base step and answers the hypotheses in one call; the second runs a REAL step per hypothesis --
`update_state` with its arrays, an evaluation -- under the same forcing `set_obstacle_stage(2, steps_per_item)`.  Everything is
compared exactly (tests/hypotheses_scene.py, same_as_real_step): winner, cost bits, n_collisions, and pred / total / collision of every
costed candidate.  N = 31 steps; obstacle counts 1, 2, 3, 4, 7, 20, 64 (every tail of the groups of four, the full 64-bit mask); 2, 3
and 5 steps per item; three grids -- fewer than 64 costed candidates, more than 128 and no multiple of 64, a few thousand.

Measured on the MI355X: the four GPU files of the pass, 41 tests, in 1.1 s."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import device_planes as dp
from tests import hypotheses_scene as hs

pytestmark = pytest.mark.gpu

CASES = [("mid", k, spi) for k in hs.KS for spi in hs.SPIS] + \
        [(g, k, spi) for g in ("small", "large") for k, spi in ((4, 2), (7, 3), (20, 5))]


@pytest.fixture(scope="module")
def engines():
    with hs.engine() as e, hs.engine() as e2:
        yield e, e2
        from frenetix_motion_planner_amd._lib import lib
        lib().fx_hypotheses_set_scratch_limit(0)


def base_step(e, inp):
    res = e.plan_step(inp)
    cost, flags = e.costs()
    assert res["best_index"] >= 0
    w = res["best_index"] - inp.shard_begin
    path = tuple(e.plane(name)[:, w] for name in ("x", "y", "theta"))
    return res, cost, flags, path


@pytest.mark.parametrize("grid,K,spi", CASES)
def test_every_hypothesis_equals_a_real_step(engines, grid, K, spi):
    e, e2 = engines
    inp = hs.make(hs.GRIDS[grid], K)
    for x in (e, e2):
        x.set_obstacle_stage(2, spi)
    res, cost, flags, path = base_step(e, inp)
    info = e.step_info()
    assert info["obstacle_kernel"] and info["obstacle_steps_per_item"] == spi
    costed = int(((flags & hs.COSTED) != 0).sum())
    # the property each grid is there for
    assert {"small": 0 < costed < 64, "mid": costed > 128 and costed % 64 != 0, "large": inp.n_candidates > 2000 and costed > 500}[grid], costed
    hyps = hs.hypotheses_of(inp, path)
    names = list(hyps)
    r = e.hypotheses([hyps[n] for n in names], pred=True, totals=True, collisions=True)
    assert e.last_hypotheses_info == dict(steps_per_item=spi, rounds=1, launches=3) and e.last_hypotheses_ms > 0.0
    # the step's own arrays reproduce the step, bit for bit
    own = names.index("own")
    ok = (flags & hs.COSTED) != 0
    assert np.array_equal(dp.bits(r["totals"][own][ok]), dp.bits(cost[ok]))
    assert np.array_equal(r["collisions"][own][ok], (flags[ok] & hs.COL) != 0)
    assert np.array_equal(dp.bits(r["pred"][own][ok]), dp.bits(e.costmap()[:, inp.cost_names.index("prediction")][ok]))
    assert r["winner"][own] == res["best_index"] and dp.bits(r["cost"][own]) == dp.bits(res["best_cost"])
    assert r["n_collisions"][own] == res["n_collisions"]
    # every hypothesis against a real step with its arrays
    e2.plan_step(inp)
    assert e2.step_info()["obstacle_kernel"] and e2.step_info()["obstacle_steps_per_item"] == spi
    for h, n in enumerate(names):
        hs.same_as_real_step(r, h, hs.real_step(e2, hyps[n]), (grid, K, spi, n))
    # the properties the cases are there for
    h = names.index("on_the_winners_path")
    assert r["winner"][h] != r["winner"][own] and r["collisions"][h][r["winner"][own]]
    h = names.index("all_absent")
    assert not r["collisions"][h].any() and r["n_collisions"][h] == 0 and np.all(r["pred"][h] == 0.0)
    h = names.index("covers_the_grid")
    n_sel = int(((flags & hs.SEL) != 0).sum())
    assert n_sel > 0 and r["winner"][h] == -1 and r["cost"][h] == np.inf and r["n_collisions"][h] == n_sel
    h = names.index("no_cholesky_factor")
    assert np.all(np.isfinite(r["pred"][h][ok])) and not np.array_equal(dp.bits(r["pred"][h][ok]), dp.bits(r["pred"][own][ok]))
    # nothing of the step was touched
    cost2, flags2 = e.costs()
    assert np.array_equal(dp.bits(cost2), dp.bits(cost)) and np.array_equal(flags2, flags)


def test_one_call_equals_single_calls_in_any_order_and_any_rounds(engines):
    from frenetix_motion_planner_amd._lib import lib
    e, _ = engines
    inp = hs.make(hs.GRIDS["mid"], 7)
    e.set_obstacle_stage(2, 3)
    _, _, _, path = base_step(e, inp)
    hyps = list(hs.hypotheses_of(inp, path).values())
    kw = dict(pred=True, totals=True, collisions=True)
    r = e.hypotheses(hyps, **kw)
    assert len(set(r["winner"].tolist())) > 1                        # (the hypotheses do not all answer the same)

    def same(a, ha, b, hb):
        assert a["winner"][ha] == b["winner"][hb] and dp.bits(a["cost"][ha]) == dp.bits(b["cost"][hb])
        assert a["n_collisions"][ha] == b["n_collisions"][hb] and np.array_equal(a["collisions"][ha], b["collisions"][hb])
        for k in ("pred", "totals"):
            nan = np.isnan(a[k][ha])
            assert np.array_equal(nan, np.isnan(b[k][hb])) and np.array_equal(dp.bits(a[k][ha][~nan]), dp.bits(b[k][hb][~nan]))

    for h, hyp in enumerate(hyps):
        same(e.hypotheses([hyp], **kw), 0, r, h)
    back = e.hypotheses(hyps[::-1], **kw)
    for h in range(len(hyps)):
        same(back, len(hyps) - 1 - h, r, h)
    # a round per hypothesis (the scratch limit of a round forced to one byte): the same answers from 3 x H launches
    lib().fx_hypotheses_set_scratch_limit(1)
    try:
        rr = e.hypotheses(hyps, **kw)
        assert e.last_hypotheses_info == dict(steps_per_item=3, rounds=len(hyps), launches=3 * len(hyps))
    finally:
        lib().fx_hypotheses_set_scratch_limit(0)
    for h in range(len(hyps)):
        same(rr, h, r, h)
    # without the rows: the same winners
    r0 = e.hypotheses(hyps)
    assert r0["pred"] is None and r0["totals"] is None and r0["collisions"] is None
    assert np.array_equal(r0["winner"], r["winner"]) and np.array_equal(dp.bits(r0["cost"]), dp.bits(r["cost"]))


def test_a_step_whose_stage_ran_inside_the_walk(engines):
    """the policy's own choice at 630 candidates: the pass answers the bits of the same step forced to (2, steps_per_item), and
    agrees with the fused step's own cost within the suite's fixed door of 1e-9 relative (tests/test_hip_parity.py).
    Measured on the MI355X: the largest relative difference is 5.1e-15."""
    e, e2 = engines
    inp = hs.make((5, 9, 13), 5)
    assert inp.n_candidates == 630
    e.set_obstacle_stage(0)
    res, cost, flags, path = base_step(e, inp)
    assert not e.step_info()["obstacle_kernel"]
    hyps = hs.hypotheses_of(inp, path)
    names = list(hyps)
    r = e.hypotheses([hyps[n] for n in names], pred=True, totals=True, collisions=True)
    spi = e.last_hypotheses_info["steps_per_item"]
    e2.set_obstacle_stage(2, spi)
    e2.plan_step(inp)
    assert e2.step_info()["obstacle_kernel"] and e2.step_info()["obstacle_steps_per_item"] == spi
    for h, n in enumerate(names):
        hs.same_as_real_step(r, h, hs.real_step(e2, hyps[n]), ("fused", n))
    ok = (flags & hs.COSTED) != 0
    own = names.index("own")
    rel = np.abs(r["totals"][own][ok] - cost[ok]) / np.abs(cost[ok])
    print("largest relative difference against the fused step's cost:", rel.max())
    assert ok.sum() > 100 and rel.max() <= 1e-9
    assert np.array_equal(r["collisions"][own][ok], (flags[ok] & hs.COL) != 0)


def test_agent_1_of_a_batch_of_three():
    inps = [hs.make((3, 5, 7), 4), hs.make(hs.GRIDS["mid"], 7, v_des=11.0), hs.make((2, 6, 8), 2)]
    sizes = [i.n_candidates for i in inps]
    assert len(set(sizes)) == 3
    with hs.engine(max_candidates=sum(sizes) + 64 * 3, max_agents=3) as eb, hs.engine() as e2:
        for x in (eb, e2):
            x.set_obstacle_stage(2, 3)
        results = eb.plan_batch(inps)
        assert eb.step_info()["obstacle_kernel"]
        w = results[1]["best_index"]
        path = tuple(eb.plane(name, agent=1)[:, w] for name in ("x", "y", "theta"))
        hyps = hs.hypotheses_of(inps[1], path)
        names = list(hyps)
        r = eb.hypotheses([hyps[n] for n in names], agent=1, pred=True, totals=True, collisions=True)
        assert r["totals"].shape == (len(names), sizes[1])
        assert r["winner"][0] == w and r["n_collisions"][0] == results[1]["n_collisions"]
        e2.plan_step(inps[1])
        for h, n in enumerate(names):
            hs.same_as_real_step(r, h, hs.real_step(e2, hyps[n]), ("batch", n))
        # the other agents answer too, each with its own K, P and candidate count
        for a in (0, 2):
            ra = eb.hypotheses([inps[a].obstacles], agent=a, totals=True)
            assert ra["totals"].shape == (1, sizes[a]) and ra["winner"][0] == results[a]["best_index"]


def test_a_sharded_agent_answers_local_indices(engines):
    e, e2 = engines
    inp = hs.make(hs.GRIDS["large"], 7)
    inp.shard = (300, 1500)
    assert inp.n_candidates == 1500 and inp.shard_begin == 300
    for x in (e, e2):
        x.set_obstacle_stage(2, 3)
    res, cost, flags, path = base_step(e, inp)
    hyps = hs.hypotheses_of(inp, path)
    names = list(hyps)
    r = e.hypotheses([hyps[n] for n in names], pred=True, totals=True, collisions=True)
    assert r["winner"][0] == res["best_index"] - 300 and 0 <= r["winner"][0] < 1500
    e2.plan_step(inp)
    for h, n in enumerate(names):
        hs.same_as_real_step(r, h, hs.real_step(e2, hyps[n]), ("shard", n))


def test_a_cost_list_without_prediction(engines):
    """the totals are the step's own sums; only the collisions are new"""
    from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
    e, e2 = engines
    weights = {k: v for k, v in DEFAULT_COST_WEIGHTS.items() if k != "prediction"}
    inp = hs.make(hs.GRIDS["mid"], 7, cost_weights=weights)
    assert "prediction" not in inp.cost_names and inp.obstacles["K"] == 7
    for x in (e, e2):
        x.set_obstacle_stage(2, 3)
    res, cost, flags, path = base_step(e, inp)
    hyps = hs.hypotheses_of(inp, path)
    names = list(hyps)
    r = e.hypotheses([hyps[n] for n in names], pred=True, totals=True, collisions=True)
    ok = (flags & hs.COSTED) != 0
    for h in range(len(names)):
        assert np.array_equal(dp.bits(r["totals"][h][ok]), dp.bits(cost[ok])) and np.all(r["pred"][h] == 0.0)
    assert r["collisions"][names.index("on_the_winners_path")][r["winner"][0]]
    e2.plan_step(inp)
    for h, n in enumerate(names):
        hs.same_as_real_step(r, h, hs.real_step(e2, hyps[n]), ("no prediction", n))
