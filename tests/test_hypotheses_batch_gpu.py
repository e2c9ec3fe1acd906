"""fx_eval_hypotheses_batch (FrenetEngine.hypotheses_batch; csrc/fx_hypotheses_batch_kernel.h): the hypotheses
pass of several agents in one call.

The rule is one sentence -- for every listed agent every output is bit for bit what fx_eval_hypotheses_agent returns for that agent
with those hypotheses on the same resident step -- so every batch answer is compared EXACTLY with the per-agent call on the same
context: winner, cost bits, n_collisions and the bits of pred, total and the collision row of every candidate.  That call is held to
real plan steps by tests/test_hypotheses_steps_gpu.py; for two agents of the first test the batch answer is also compared with a
real `update_state` + step on a second engine (hypotheses_scene.real_step / same_as_real_step), so the chain ends outside the
hypotheses code.  N = 31 steps: the last chunk is short for 2, 3 and 5 steps per item.  Scenes of an exact candidate count are cut
from the sampling matrix of an `as_matrix=True` scene (as tests/rescore_rows.py cuts its scenes).

Measured on the MI355X: the three GPU files of the batch call, 16 tests, in 3.5 s; the ten of this file in 0.9 s."""
import copy

import numpy as np
import pytest

from tests import device_planes as dp
from tests import hypotheses_scene as hs

pytestmark = pytest.mark.gpu

KW = dict(pred=True, totals=True, collisions=True)
# the mixed context: the edges of the 64-candidate tile and of the 256-candidate finish tile, ragged K and H
MIXED_C = (1, 63, 64, 65, 257)
MIXED_K = (1, 4, 7, 20, 2)
MIXED_NAMES = (("own",),
               ("own", "on_the_winners_path", "covers_the_grid"),
               ("own", "on_the_winners_path", "shorter_than_the_horizon", "at_most_two_steps", "no_cholesky_factor", "all_absent", "covers_the_grid"),
               ("own", "all_absent"),
               ("own", "on_the_winners_path", "all_absent", "covers_the_grid", "shorter_than_the_horizon"))
_BASE = {}


def scene(n, K, **kw):
    """PlanInputs of exactly n candidates and K obstacles"""
    key = (K, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _BASE:
        _BASE[key] = hs.make(hs.GRIDS["mid"], K, as_matrix=True, **kw)
    inp = copy.copy(_BASE[key])
    inp.sampling_matrix = np.ascontiguousarray(inp.sampling_matrix[:n])
    assert inp.n_candidates == n and inp.obstacles["K"] == K
    return inp


def path_of(e, agent, result, inp):
    """(x, y, theta) of the agent's winner, or of candidate 0 where the step has none: the path an obstacle is moved onto"""
    w = max(result["best_index"] - inp.shard_begin, 0)
    return tuple(e.plane(name, agent=agent)[:, w] for name in ("x", "y", "theta"))


def same(a, b, what=""):
    """two answers of the same agent, every output bit for bit"""
    assert np.array_equal(a["winner"], b["winner"]), what
    assert np.array_equal(dp.bits(a["cost"]), dp.bits(b["cost"])), what
    assert np.array_equal(a["n_collisions"], b["n_collisions"]), what
    for k in ("pred", "totals"):
        assert (a[k] is None) == (b[k] is None), what
        if a[k] is not None:
            assert a[k].shape == b[k].shape and np.array_equal(dp.bits(a[k]), dp.bits(b[k])), (what, k)
    assert (a["collisions"] is None) == (b["collisions"] is None), what
    if a["collisions"] is not None:
        assert a["collisions"].dtype == np.bool_ and np.array_equal(a["collisions"], b["collisions"]), what


def loop_of(e, sets, agents, **kw):
    """the per-agent loop a hypotheses_batch call replaces, on the same context"""
    return [e.hypotheses(s, agent=a, **kw) for s, a in zip(sets, agents)]


def same_as_loop(e, sets, agents, what="", **kw):
    got = e.hypotheses_batch(sets, agents=agents, **kw)
    want = loop_of(e, sets, agents, **kw)
    assert len(got) == len(want) == len(agents)
    for g, w, a in zip(got, want, agents):
        same(g, w, (what, a))
    return got


@pytest.fixture(scope="module")
def mixed():
    """one context of six agents: the five of MIXED_C and one of 65 candidates and 64 obstacles, which sizes the item launch's LDS
    for the others"""
    inps = [scene(n, K) for n, K in zip(MIXED_C, MIXED_K)] + [scene(65, 64)]
    with hs.engine(max_candidates=sum(i.n_candidates for i in inps) + 64 * len(inps), max_agents=len(inps)) as e, hs.engine() as e2:
        yield e, e2, inps
        from frenetix_motion_planner_amd._lib import lib
        lib().fx_hypotheses_set_scratch_limit(0)


def step_and_sets(e, inps, spi):
    e.set_obstacle_stage(2, spi)
    results = e.plan_batch(inps)
    info = e.step_info()
    assert info["obstacle_kernel"] and info["obstacle_steps_per_item"] == spi
    hyps = [hs.hypotheses_of(inp, path_of(e, a, results[a], inp)) for a, inp in enumerate(inps)]
    names = list(MIXED_NAMES) + [("own",)]
    assert [len(n) for n in names[:5]] == [1, 3, 7, 2, 5]
    return results, [[hyps[a][n] for n in names[a]] for a in range(len(inps))], names


@pytest.mark.parametrize("spi", hs.SPIS)
def test_every_agent_equals_its_own_call(mixed, spi):
    e, e2, inps = mixed
    results, sets, names = step_and_sets(e, inps, spi)
    agents = list(range(len(inps)))
    got = same_as_loop(e, sets, agents, spi, **KW)
    n_pairs = sum(len(s) for s in sets)
    assert e.last_hypotheses_info == dict(steps_per_item=spi, rounds=1, launches=3) and e.last_hypotheses_ms > 0.0
    for a, (g, inp) in enumerate(zip(got, inps)):
        assert g["totals"].shape == (len(sets[a]), inp.n_candidates) and g["winner"].shape == (len(sets[a]),)
        own = names[a].index("own")
        assert g["winner"][own] == results[a]["best_index"] and g["n_collisions"][own] == results[a]["n_collisions"]
        if results[a]["best_index"] >= 0:
            assert dp.bits(g["cost"][own]) == dp.bits(results[a]["best_cost"])
    # the test's own preconditions: the hypotheses do not all answer as the step did, some collide, some leave nothing eligible
    winners = [(int(w), results[a]["best_index"]) for a, g in enumerate(got) for w in g["winner"]]
    assert len(winners) == n_pairs and any(w != own for w, own in winners)
    assert any((g["n_collisions"] > 0).any() for g in got)
    assert any(((g["winner"] == -1) & (g["cost"] == np.inf)).any() for g in got)
    # two agents against real steps on a second engine: the chain ends outside the hypotheses code
    e2.set_obstacle_stage(2, spi)
    for a in (2, 4):
        e2.plan_step(inps[a])
        assert e2.step_info()["obstacle_kernel"] and e2.step_info()["obstacle_steps_per_item"] == spi
        for h, hyp in enumerate(sets[a]):
            hs.same_as_real_step(got[a], h, hs.real_step(e2, hyp), (spi, a, names[a][h]))
    # without the rows: the same winners; the arrays are views of the call's concatenated ones
    plain = e.hypotheses_batch(sets)
    for g, p in zip(got, plain):
        assert p["pred"] is None and p["totals"] is None and p["collisions"] is None
        assert np.array_equal(p["winner"], g["winner"]) and np.array_equal(dp.bits(p["cost"]), dp.bits(g["cost"]))
    assert all(p["winner"].base is plain[0]["winner"].base for p in plain) and all(g["totals"].base is not None for g in got)


def test_subsets_in_any_order(mixed):
    e, _, inps = mixed
    _, sets, _ = step_and_sets(e, inps, 3)
    full = e.hypotheses_batch(sets, **KW)
    for agents in ((4, 0, 2), (3,), (5, 1)):
        got = same_as_loop(e, [sets[a] for a in agents], list(agents), agents, **KW)
        for g, a in zip(got, agents):
            same(g, full[a], ("subset", agents, a))
    assert e.hypotheses_batch([]) == [] and e.hypotheses_batch([], agents=[]) == []


def test_rounds_cut_agents_and_share_agents(mixed):
    """a forced scratch limit: 100 000 bytes cut agent 1's and agent 2's hypotheses across rounds and let agents 0 and 1, and 1 and
    2, share one; 400 000 bytes put three agents into each of the first two rounds and leave the agent of 64 obstacles alone
    (tests/test_hypotheses_batch_plan.py holds the same shapes to these 11 and 4 rounds); one byte is one pair per round"""
    from frenetix_motion_planner_amd._lib import lib
    e, _, inps = mixed
    _, sets, _ = step_and_sets(e, inps, 3)
    agents = list(range(len(inps)))
    n_pairs = sum(len(s) for s in sets)
    want = e.hypotheses_batch(sets, **KW)
    assert e.last_hypotheses_info["rounds"] == 1
    try:
        for limit, rounds in ((100_000, 11), (400_000, 4), (1, n_pairs)):
            lib().fx_hypotheses_set_scratch_limit(limit)
            got = e.hypotheses_batch(sets, agents=agents, **KW)
            assert e.last_hypotheses_info == dict(steps_per_item=3, rounds=rounds, launches=3 * rounds), limit
            for g, w, a in zip(got, want, agents):
                same(g, w, ("rounds", limit, a))
    finally:
        lib().fx_hypotheses_set_scratch_limit(0)


def test_interleaved_with_the_per_agent_call(mixed):
    """per-agent call, batch call, per-agent call: the same bits each time; the two calls share one grow-only block"""
    e, _, inps = mixed
    _, sets, _ = step_and_sets(e, inps, 5)
    agents = [1, 2, 4]
    e.hypotheses_batch(sets, **KW)                               # (the block has its size for everything below)
    b0 = e.device_bytes
    first = loop_of(e, [sets[a] for a in agents], agents, **KW)
    assert e.last_hypotheses_info["steps_per_item"] == 5
    batch = e.hypotheses_batch([sets[a] for a in agents], agents=agents, **KW)
    again = loop_of(e, [sets[a] for a in agents], agents, **KW)
    for f, b, g, a in zip(first, batch, again, agents):
        same(b, f, ("interleaved", a))
        same(g, f, ("interleaved again", a))
    assert e.device_bytes == b0


@pytest.fixture(scope="module")
def many():
    """129 agents of 63 to 130 candidates, two obstacle counts"""
    inps = [scene(63 + (7 * i) % 68, (2, 5)[i % 2]) for i in range(129)]
    with hs.engine(max_candidates=sum(i.n_candidates for i in inps) + 64 * len(inps), max_agents=len(inps)) as e:
        e.set_obstacle_stage(2, 3)
        results = e.plan_batch(inps)
        assert e.step_info()["obstacle_kernel"]
        hyps = [hs.hypotheses_of(inps[a], path_of(e, a, results[a], inps[a])) for a in (0, 1)]
        pick = (("on_the_winners_path",), ("own", "all_absent"), ("covers_the_grid",), ("no_cholesky_factor", "on_the_winners_path"))
        sets = [[hyps[i % 2][n] for n in pick[i % 4]] for i in range(len(inps))]
        yield e, inps, results, sets


@pytest.mark.parametrize("A", (65, 129))
def test_more_rows_than_a_wave_has_lanes(many, A):
    e, inps, results, sets = many
    assert min(i.n_candidates for i in inps) == 63 and max(i.n_candidates for i in inps) == 130
    assert {len(s) for s in sets} == {1, 2}
    agents = list(range(A))
    got = same_as_loop(e, sets[:A], agents, A, **KW)
    assert e.last_hypotheses_info == dict(steps_per_item=3, rounds=1, launches=3)
    assert len({int(g["winner"][0]) for g in got}) > 1 and any((g["winner"] == -1).any() for g in got)
    sub = [A - 1, 64, 0, 63, 65] if A > 65 else [A - 1, 0, 63]
    for g, a in zip(same_as_loop(e, [sets[a] for a in sub], sub, ("subset", A), **KW), sub):
        same(g, got[a], ("subset of many", a))


def test_the_policys_own_fused_step():
    """a small batch whose obstacle stage ran inside the walk: the batch call answers what the per-agent call answers"""
    inps = [scene(130, 4), scene(65, 2), scene(257, 7)]
    with hs.engine(max_candidates=sum(i.n_candidates for i in inps) + 64 * 3, max_agents=3) as e:
        e.set_obstacle_stage(0)
        results = e.plan_batch(inps)
        assert not e.step_info()["obstacle_kernel"]
        hyps = [hs.hypotheses_of(inp, path_of(e, a, results[a], inp)) for a, inp in enumerate(inps)]
        sets = [list(h.values())[:3 + a] for a, h in enumerate(hyps)]
        got = same_as_loop(e, sets, [0, 1, 2], "fused", **KW)
        assert all(g["winner"][0] == r["best_index"] for g, r in zip(got, results))


def test_a_cost_list_without_prediction():
    """the totals are the steps' own sums; only the collisions are new"""
    from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
    weights = {k: v for k, v in DEFAULT_COST_WEIGHTS.items() if k != "prediction"}
    inps = [scene(130, 4, cost_weights=weights), scene(63, 7, cost_weights=weights)]
    assert all("prediction" not in i.cost_names for i in inps)
    with hs.engine(max_candidates=sum(i.n_candidates for i in inps) + 64 * 2, max_agents=2) as e:
        e.set_obstacle_stage(2, 3)
        results = e.plan_batch(inps)
        hyps = [hs.hypotheses_of(inp, path_of(e, a, results[a], inp)) for a, inp in enumerate(inps)]
        sets = [[h["own"], h["on_the_winners_path"], h["all_absent"]] for h in hyps]
        got = same_as_loop(e, sets, [0, 1], "no prediction", **KW)
        for a, g in enumerate(got):
            cost, flags = e.costs(a)
            ok = (flags & hs.COSTED) != 0
            assert np.all(g["pred"] == 0.0) and all(np.array_equal(dp.bits(t[ok]), dp.bits(cost[ok])) for t in g["totals"])
