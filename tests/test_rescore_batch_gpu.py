"""fx_rescore_batch (FrenetEngine.rescore_batch; csrc/fx_rescore_batch_kernel.h): the re-score of several agents
of a context in one call, held to the per-agent call on the SAME context -- every entry takes the launch shape it would have alone,
so winner and cost are `array_equal` (the cost bit for bit).

  * entries of different shapes: agents of 1, 63, 64, 65 and 257 candidates with W = 65, 1, 64, 63, 2 vectors -- both regimes in one
    call, and each regime forced for all; a subset given out of order; some agents with external rows and some without;
  * more agents than a wave has lanes: A = 65 and 129 small agents (63 to 130 candidates, the scenes of
    tests/test_many_agents_gpu.py), ragged W, the subset (A - 1, 64, 0, 63, 65); the agent whose step returns nothing answers
    -1 / +inf for every vector;
  * refusals leave the context usable."""
import ctypes as C

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import rescore_planes as rp
from tests import rescore_rows as rr

pytestmark = pytest.mark.gpu

SHAPES = ((1, 65), (63, 1), (64, 64), (65, 63), (257, 2))    # (candidates, vectors) per agent


def weights_of(inp, n_vec, resp=False, seed=0):
    return rp.weight_vectors(n_vec, len(inp.cost_names) + int(resp)) * (1.0 + 0.125 * seed)


@pytest.fixture(scope="module")
def shapes():
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inps = [rr.scene(n, "plain") for n, _ in SHAPES]
    e = FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in inps), max_steps=inps[0].N, max_agents=len(inps))
    e.plan_batch(inps)
    for a, inp in enumerate(inps):      # planes of the test's own: ties, NaN and infinities, flag reasons
        raw, flags = rp.plane(rp.PLANES[a % len(rp.PLANES)], inp.n_candidates, len(inp.cost_names))
        rp.write_rows(e, a, raw, flags)
    yield e, inps
    lib().fx_rescore_set_regime(0)
    e.close()


def test_both_regimes_in_one_call(shapes):
    from frenetix_motion_planner_amd._lib import lib
    e, inps = shapes
    agents = list(range(len(inps)))
    W = [weights_of(inp, w, seed=a) for a, (inp, (_, w)) in enumerate(zip(inps, SHAPES))]
    regimes = [lib().fx_rescore_regime(n, w) for n, w in SHAPES]
    assert regimes == [rp.VECTOR, rp.LANE, rp.VECTOR, rp.LANE, rp.LANE]
    try:
        for forced in (0, rp.LANE, rp.VECTOR):
            lib().fx_rescore_set_regime(forced)
            got = rr.same_as_loop(e, W, agents, what=("all", forced))
            assert [len(g["winner"]) for g in got] == [w for _, w in SHAPES]
            assert e.last_rescore_ms > 0.0
    finally:
        lib().fx_rescore_set_regime(0)
    # the planes are what they are for every agent: the reference of the per-agent tests holds the batch too
    for a, inp in enumerate(inps):
        raw, flags = rp.plane(rp.PLANES[a % len(rp.PLANES)], inp.n_candidates, len(inp.cost_names))
        win, cost, _ = rr.expected(raw, flags, W[a], inp._cost_id, bool(e.step_info()["obstacle_kernel"]))
        rr.same_result(got[a], win, cost, ("reference", a))


def test_a_subset_out_of_order(shapes):
    e, inps = shapes
    agents = [4, 0, 2]
    W = [weights_of(inps[a], w, seed=7 + a) for a, w in zip(agents, (3, 64, 1))]
    rr.same_as_loop(e, W, agents, what="subset")
    rr.same_as_loop(e, W[:1], agents[:1], what="one")
    assert e.rescore_batch([], agents=[]) == []


def test_some_agents_with_rows_and_some_without(shapes):
    from frenetix_motion_planner_amd._lib import lib
    e, inps = shapes
    agents = [3, 1, 4, 0, 2]
    has = {3: (True, True), 1: (False, False), 4: (False, True), 0: (True, False), 2: (False, False)}
    n_vec = {3: 63, 1: 2, 4: 64, 0: 1, 2: 65}
    pred = [rr.external_row("non_finite" if a == 3 else "plain", inps[a].n_candidates, 10 + a) if has[a][0] else None for a in agents]
    resp = [rr.external_row("plain", inps[a].n_candidates, 20 + a) if has[a][1] else None for a in agents]
    W = [weights_of(inps[a], n_vec[a], resp=has[a][1], seed=a) for a in agents]
    try:
        for forced in (0, rp.LANE, rp.VECTOR):
            lib().fx_rescore_set_regime(forced)
            got = rr.same_as_loop(e, W, agents, pred, resp, what=("rows", forced))
    finally:
        lib().fx_rescore_set_regime(0)
    # ... and the NumPy sum of the effective list
    for g, a, w, p, r in zip(got, agents, W, pred, resp):
        inp = inps[a]
        raw, flags = rp.plane(rp.PLANES[a % len(rp.PLANES)], inp.n_candidates, len(inp.cost_names))
        win, cost, _ = rr.expected(raw, flags, w, inp._cost_id, bool(e.step_info()["obstacle_kernel"]), p, r)
        rr.same_result(g, win, cost, ("reference", a))


def test_refusals_leave_the_context_usable(shapes):
    from frenetix_motion_planner_amd._lib import lib
    e, inps = shapes
    W = [weights_of(inps[a], 2, seed=a) for a in (0, 1)]
    good = rr.same_as_loop(e, W, [0, 1])
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def raw_call(agents, n_vec, w, pred=None, win=True, cost=True):
        agents, n_vec = np.array(agents, np.int32), np.array(n_vec, np.int32)
        out_w, out_c = np.zeros(max(int(np.abs(n_vec).sum()), 1), np.int64), np.zeros(max(int(np.abs(n_vec).sum()), 1))
        return lib().fx_rescore_batch(e._ctx, len(agents), ptr(agents), ptr(n_vec), ptr(w), pred, None, ptr(out_w) if win else None,
                                      ptr(out_c) if cost else None)

    def still_answers():
        for g, h in zip(e.rescore_batch(W, agents=[0, 1]), good):
            rr.same_result(g, h["winner"], h["cost"])

    w = np.ascontiguousarray(np.concatenate([x.ravel() for x in W]))
    INV, CAP = _abi.FX_ERR_INVALID_ARGUMENT, _abi.FX_ERR_CAPACITY
    assert raw_call([0, 1], [2, 2], w) == _abi.FX_OK
    assert raw_call([0, 5], [2, 2], w) == INV and raw_call([0, -1], [2, 2], w) == INV          # out of range
    assert raw_call([1, 1], [2, 2], w) == INV and b"twice" in lib().fx_last_error()             # listed twice
    assert raw_call([0, 1], [2, 0], w) == INV and b"agent 1" in lib().fx_last_error()           # n_vec < 1
    assert raw_call([0, 1], [2, 2], None) == INV and raw_call([0, 1], [2, 2], w, win=False) == INV and raw_call([0, 1], [2, 2], w, cost=False) == INV
    still_answers()
    for bad in (0.0, np.nan, np.inf):
        wb = w.copy()
        wb[-1] = bad
        assert raw_call([0, 1], [2, 2], wb) == INV and b"agent 1" in lib().fx_last_error()
        with pytest.raises(ValueError):
            e.rescore_batch([W[0], wb[-W[1].size:].reshape(W[1].shape)], agents=[0, 1])
    big = np.ones((_abi.FX_RESCORE_MAX_VECTORS + 1) * 5 + 10)
    assert raw_call([0, 1], [2, _abi.FX_RESCORE_MAX_VECTORS + 1], big) == CAP and b"agent 1" in lib().fx_last_error()
    still_answers()
    with pytest.raises(ValueError):
        e.rescore_batch(W, agents=[0])                     # two weight sets, one agent
    with pytest.raises(ValueError):
        e.rescore_batch(W, agents=[0, 1], pred=[np.zeros(3), None])      # a row of the wrong length
    with pytest.raises(ValueError):
        e.rescore_batch([W[0], np.ones((2, 6))], agents=[0, 1])         # six weights without a responsibility row
    still_answers()


def test_a_prediction_row_needs_a_prediction_term():
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
    w = {k: v for k, v in DEFAULT_COST_WEIGHTS.items() if k != "prediction"}
    inp = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(3, 5, 5), n_obstacles=0, cost_weights=w)
    n = inp.n_candidates
    with FrenetEngine(max_candidates=n + 64, max_steps=inp.N) as e:
        res = e.plan_step(inp)
        own = np.array([inp._cost_w])
        with pytest.raises(ValueError, match="prediction"):
            e.rescore(own, pred=np.zeros(n))
        with pytest.raises(ValueError, match="agent 0"):
            e.rescore_batch([own], pred=[np.zeros(n)])
        # a responsibility row is legal there: behind the last term but `velocity_offset`
        assert rr.resp_at(inp._cost_id) == len(inp.cost_names) - 1
        r = e.rescore(np.array([list(inp._cost_w[:-1]) + [1.0, inp._cost_w[-1]]]), resp=np.zeros(n), totals=True)
        cost, flags = e.costs()
        costed = (flags & _abi.FX_FLAG_COSTED) != 0
        assert r["winner"][0] == res["best_index"] and np.array_equal(r["totals"][0][costed], cost[costed])   # (+ 1.0 * 0.0: the same value)
        assert e.rescore_batch([own])[0]["winner"][0] == res["best_index"]


# ---- more agents than a wave has lanes ----
@pytest.fixture(scope="module", params=(65, 129), ids=lambda A: f"A{A}")
def many(request):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from tests import test_many_agents_gpu as ma
    A = request.param
    inps = [ma.make(a, ma._hip_hulls()) for a in range(A)]
    e = FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in inps), max_agents=A)
    res = e.plan_batch(inps)
    yield A, e, inps, res
    e.close()


def ragged(a):
    return (1, 2, 5, 63, 64, 65, 3, 70)[a % 8]


def test_more_agents_than_a_wave_has_lanes(many):
    from tests import test_many_agents_gpu as ma
    A, e, inps, res = many
    assert {i.n_candidates for i in inps} == {63, 64, 65, 130}
    W = [weights_of(inps[a], ragged(a), seed=a) for a in range(A)]
    got = rr.same_as_loop(e, W, list(range(A)), what=A)
    # vector 0 of every agent is all ones, not the step's weights; the step's own weights reproduce the step
    own = e.rescore_batch([np.array([inp._cost_w]) for inp in inps])
    for a in range(A):
        assert own[a]["winner"][0] == (res[a]["best_index"] if res[a]["best_index"] >= 0 else -1), a
    nothing = got[ma.NOTHING_RETURNED]
    assert np.all(nothing["winner"] == -1) and np.all(nothing["cost"] == np.inf) and len(nothing["winner"]) == ragged(ma.NOTHING_RETURNED)
    assert sum(int((g["winner"] >= 0).all()) for g in got) > A // 2
    sub = ma.subset_of(A)
    assert sub[:1] == [A - 1] and set(sub) >= {64, 0, 63}
    rr.same_as_loop(e, [W[a] for a in sub], sub, what=("subset", A))
    pred = [rr.external_row("plain", inps[a].n_candidates, a) for a in sub]
    resp = [rr.external_row("plain", inps[a].n_candidates, 100 + a) for a in sub]
    rr.same_as_loop(e, [weights_of(inps[a], ragged(a + 3), resp=True, seed=a) for a in sub], sub, pred=pred, resp=resp, what=("subset with rows", A))
