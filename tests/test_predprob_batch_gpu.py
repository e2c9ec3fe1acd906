"""The collision-probability pass over a whole agent batch in one call (fx_eval_prediction_prob_batch) against
the per-agent call on the same context -- bit for bit, whichever agents share a call, however the candidates are cut into rounds
and the steps into chunks -- and, independently of that shared code, against the NumPy restatement (tests/predprob_restatement.py)
at the bound of tests/test_predprob_gpu.py: every term of a sum is a probability held to 1e-12, a cost of K sums of S - 1 terms
stays within (K (S - 1) + 1) 1e-12 absolute.

Shapes: the smallest at which the mapping of (agent, tile, chunk, obstacle) can go wrong.  synthetic.make_inputs adds the ego's
own lateral offset to the n_d lateral samples, so a grid (n_t, n_v, n_d) has n_t n_v (n_d + 1) candidates; the grids below are the
nearest ones it accepts that give the intended counts:
  agent 0: (3, 5, 3)  =   60 candidates, K = 0          one partial tile and no item at all
  agent 1: (4, 8, 7)  =  256 candidates, K = 1, 2.0 s   exact tiles, S = 21: other chunk counts in the same launch
  agent 2: (5, 7, 8)  =  315 candidates, K = 8          a tile remainder
  agent 3: (8, 16, 16) = 2 176 candidates, K = 20, seed 7: the grid and scene of tests/test_predprob_gpu.py, some predictions S - 7 long
  agent 4: (2, 4, 4)  =   40 candidates, K = 5          less than a tile
Every agent has its own ego footprint."""
import ctypes as C

import numpy as np
import pytest

from tests import predprob_restatement as pp
from tests.test_risk_gpu import _predictions

pytestmark = pytest.mark.gpu

EGO_L, EGO_W = 4.508, 1.61
COSTED, SELECTABLE = 0x10, 0x20
SHAPES = [dict(grid=(3, 5, 3), K=0, seed=1), dict(grid=(4, 8, 7), K=1, seed=2, horizon=2.0), dict(grid=(5, 7, 8), K=8, seed=3),
          dict(grid=(8, 16, 16), K=20, seed=7), dict(grid=(2, 4, 4), K=5, seed=5)]
COUNTS = [60, 256, 315, 2176, 40]
KEYS = ("prob", "total")


def _make(shape, **kw):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    args = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=shape["grid"], n_obstacles=4, horizon=shape.get("horizon", 3.0))
    args.update(kw)
    return synthetic.make_inputs(**args)


def _engine(n_agents=33, candidates=8192):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    return FrenetEngine(max_candidates=candidates, device=0, max_agents=n_agents)


def _tables(preds):
    from frenetix_motion_planner_amd import risk
    return risk.obstacle_tables(preds, {k: "car" for k in preds})


def _scene(eng, a, shape):
    """agent a's read-back planes and flags, and its K obstacles along its own candidates (set on the engine)"""
    _, flags = eng.costs(a)
    planes = {n: eng.plane(n, a).T.copy() for n in ("x", "y", "theta", "v")}
    preds = _predictions(planes, flags, np.random.default_rng(shape["seed"]), n_obs=shape["K"])[0] if shape["K"] else {}
    eng.set_risk_obstacles(_tables(preds), a)
    return planes, flags, preds


def _same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    assert got["best_index"] == want["best_index"], what
    assert np.array_equal(np.float64(got["best_cost"]).view(np.uint64), np.float64(want["best_cost"]).view(np.uint64)), what


def _dims(n):
    return [EGO_L + 0.1 * a for a in range(n)], [EGO_W + 0.02 * a for a in range(n)]


@pytest.fixture(scope="module")
def ctx():
    """one context of five agents with their scenes, the per-agent calls and the batched call -- computed once, left unchanged"""
    inps = [_make(s) for s in SHAPES]
    assert [i.n_candidates for i in inps] == COUNTS and [i.n_samples for i in inps] == [31, 21, 31, 31, 31]
    eng = _engine()
    eng.plan_batch(inps)
    scenes = [_scene(eng, a, s) for a, s in enumerate(SHAPES)]
    ln, wd = _dims(5)
    solo = [eng.prediction_probability(ln[a], wd[a], agent=a) for a in range(5)]
    batch = eng.prediction_probability_batch(ln, wd)
    yield eng, inps, scenes, solo, batch
    eng.close()


def test_batch_equals_agents_alone(ctx):
    eng, inps, scenes, solo, batch = ctx
    ln, wd = _dims(5)
    assert len(batch) == 5
    for a, (shape, (planes, flags, preds)) in enumerate(zip(SHAPES, scenes)):
        K, S = shape["K"], inps[a].n_samples
        _same(batch[a], solo[a], a)
        assert batch[a]["prob"].shape == batch[a]["total"].shape == (COUNTS[a],)
        ids = np.nonzero(flags & COSTED)[0]
        rest = np.setdiff1d(np.arange(COUNTS[a]), ids)
        assert len(ids) > 0 and np.all(np.isnan(batch[a]["prob"][rest])) and np.all(np.isnan(batch[a]["total"][rest]))
        assert not np.isnan(batch[a]["prob"][ids]).any()
        assert batch[a]["best_index"] == pp.best_index(batch[a]["total"], flags), a
        positive = int((batch[a]["prob"][ids] > 0).sum())
        print(f"agent {a}: C = {COUNTS[a]}, S = {S}, K = {K}, {len(ids)} costed, {positive} with a positive sum")
        if K == 0:
            assert np.all(batch[a]["prob"][ids] == 0.0)
        else:
            assert positive > 0, a
        if K >= 8:
            want, _, _ = pp.prediction_probability(planes["x"][ids], planes["y"][ids], planes["theta"][ids], preds, ln[a], wd[a])
            err = float(np.abs(batch[a]["prob"][ids] - want).max())
            print(f"  against the restatement: largest error {err:.3e} (bound {(K * (S - 1) + 1) * 1e-12:.1e})")
            assert err <= (K * (S - 1) + 1) * 1e-12
        if a == 3:
            assert positive > len(ids) // 4, "too few candidates near an obstacle"
            assert {len(p["pos_list"]) for p in preds.values()} == {S - 1, S - 7}


def test_subsets_and_order(ctx):
    eng, inps, scenes, solo, batch = ctx
    ln, wd = _dims(5)
    for agents in ([3, 1], [2], [4, 0, 3], None):
        lst = list(range(5)) if agents is None else agents
        res = eng.prediction_probability_batch([ln[a] for a in lst], [wd[a] for a in lst], agents=agents)
        assert len(res) == len(lst)
        for r, a in zip(res, lst):
            _same(r, solo[a], (agents, a))
        # the views lie in the concatenated arrays at the sums of C of the agents in front
        base = res[0]["prob"].base
        assert base is not None and all(r["prob"].base is base for r in res)
        off = np.concatenate([[0], np.cumsum([COUNTS[a] for a in lst])])
        first = res[0]["prob"].__array_interface__["data"][0]
        assert [r["prob"].__array_interface__["data"][0] - first for r in res] == [8 * int(o) for o in off[:-1]]


def test_partition_independence(ctx):
    """other rounds, other chunks, the same bits.  Scratch per candidate: agent 1 160 bytes, agent 2 1 920, agent 3 4 800, agent 4
    1 200 (agent 0 has no item).  At 368 640 bytes -- three tiles of agent 2 -- agent 1 and the first two tiles of agent 2 share round
    0, agent 2 ends in round 1, agent 3 takes a round per tile and agent 4 a last one; at 1 MiB agent 3 starts in agent 2's round,
    goes on three tiles a round, and agent 4 joins its last."""
    from frenetix_motion_planner_amd._lib import lib
    eng, inps, scenes, solo, batch = ctx
    ln, wd = _dims(5)
    try:
        for limit in (3 * 64 * 1920, 1 << 20, 1):
            lib().fx_predprob_set_scratch_limit(limit)
            for a, r in enumerate(eng.prediction_probability_batch(ln, wd)):
                _same(r, solo[a], (limit, a))
        lib().fx_predprob_set_scratch_limit(0)
        for cs in (1, 7, 30):
            lib().fx_predprob_set_chunk_steps(cs)
            for a, r in enumerate(eng.prediction_probability_batch(ln, wd)):
                _same(r, solo[a], (cs, a))
        lib().fx_predprob_set_chunk_steps(7)
        lib().fx_predprob_set_scratch_limit(1 << 20)
        for a, r in enumerate(eng.prediction_probability_batch(ln, wd)):
            _same(r, solo[a], ("both", a))
    finally:
        lib().fx_predprob_set_chunk_steps(0)
        lib().fx_predprob_set_scratch_limit(0)
    one, two = eng.prediction_probability_batch(ln, wd), eng.prediction_probability_batch(ln, wd)
    for a in range(5):
        _same(one[a], two[a], a)
        _same(one[a], batch[a], a)
    assert eng.last_predprob_ms > 0


@pytest.mark.parametrize("case", ["split", "fused"])
def test_step_source_is_the_step_cost(case):
    """source="step": every agent's total is its step's cost bit for bit -- for a step whose obstacle stage ran as its own kernel
    (the sum closed there) and for one that ran it inside the walk"""
    inps = [_make(s) for s in SHAPES[1:4]]
    with _engine(3) as eng:
        eng.set_obstacle_stage(2 if case == "split" else 1)
        eng.plan_batch(inps)
        for a in range(3):
            eng.set_risk_obstacles(_tables({}), a)
        info = eng.step_info()
        print(case, info)
        assert bool(info["obstacle_kernel"]) == (case == "split")
        res = eng.prediction_probability_batch(EGO_L, EGO_W, source="step")
        for a, r in enumerate(res):
            cost, flags = eng.costs(a)
            ids = np.nonzero(flags & COSTED)[0]
            n_pred = inps[a].cost_names.index("prediction")
            assert len(ids) > 30 and np.array_equal(r["total"][ids], cost[ids]), (case, a)
            assert np.array_equal(r["prob"][ids], eng.costmap(a)[ids, n_pred])
            _same(r, eng.prediction_probability(EGO_L, EGO_W, agent=a, source="step"), a)


def test_33_agents():
    """32 of the smallest shape and one of the largest: more rows than half a wave looks up at once, and no fixed-size table"""
    shapes = [SHAPES[0]] * 20 + [SHAPES[3]] + [SHAPES[0]] * 12
    inps = [_make(s, v0=8.0 + 0.1 * a) for a, s in enumerate(shapes)]
    with _engine() as eng:
        eng.plan_batch(inps)
        for a, s in enumerate(shapes):
            _scene(eng, a, dict(s, K=3 if a != 20 else 20))
        ln, wd = _dims(33)
        res = eng.prediction_probability_batch(ln, wd)
        some = eng.prediction_probability_batch([ln[a] for a in (32, 20, 0)], [wd[a] for a in (32, 20, 0)], agents=[32, 20, 0])
        assert len(res) == 33
        positive = 0
        for a in range(33):
            want = eng.prediction_probability(ln[a], wd[a], agent=a)
            _same(res[a], want, a)
            positive += int(np.nansum(want["prob"] > 0) > 0)
        print(f"{positive} of 33 agents with a positive sum")
        assert np.nansum(res[20]["prob"] > 0) > 0 and positive > 16
        for r, a in zip(some, (32, 20, 0)):
            _same(r, res[a], a)


def _raw(eng, agents, source=0, length=EGO_L, n=None):
    """the library's call with sentinel-filled outputs: (status, message, prob, total, best_index, best_cost)"""
    from frenetix_motion_planner_amd import _abi
    from frenetix_motion_planner_amd._lib import lib
    n = len(agents) if n is None else n
    rows = sum(eng._inputs[a].n_candidates for a in agents if 0 <= a < len(eng._inputs))
    prob, total = np.full(max(rows, 1), 7.25), np.full(max(rows, 1), 7.25)
    bi, bc = np.full(max(len(agents), 1), 7, np.int64), np.full(max(len(agents), 1), 7.25)
    params = (_abi.FxPredProbParams * max(len(agents), 1))(*[_abi.FxPredProbParams(length, EGO_W, source) for _ in agents])
    out = _abi.FxPredProbBatchOutputs(prob.ctypes.data, total.ctypes.data, bi.ctypes.data, bc.ctypes.data)
    ids = np.ascontiguousarray(agents, np.int32)
    rc = lib().fx_eval_prediction_prob_batch(eng._ctx, n, ids.ctypes.data_as(C.POINTER(C.c_int32)), params, C.byref(out))
    return rc, lib().fx_last_error().decode(), prob, total, bi, bc


def _untouched(r):
    return np.all(r[2] == 7.25) and np.all(r[3] == 7.25) and np.all(r[4] == 7) and np.all(r[5] == 7.25)


def test_refusals_on_the_shared_context(ctx):
    from frenetix_motion_planner_amd import _abi
    eng, inps, scenes, solo, batch = ctx
    ln, wd = _dims(5)
    before = eng.device_bytes
    for name, r, word in (("duplicate", _raw(eng, [1, 2, 1]), "agent 1 listed twice"), ("out of range", _raw(eng, [0, 5]), "agent 5"),
                          ("negative", _raw(eng, [0, -1]), "agent -1"), ("too many", _raw(eng, [0, 1, 2, 3, 4, 4], n=6), ""),
                          ("unknown source", _raw(eng, [2, 3], source=9), "agent 2"), ("length", _raw(eng, [4, 3], length=0.0), "agent 4")):
        assert r[0] == _abi.FX_ERR_INVALID_ARGUMENT and word in r[1] and _untouched(r), (name, r[:2])
    r = _raw(eng, [0, 1], n=0)
    assert r[0] == _abi.FX_OK and _untouched(r)
    assert eng.device_bytes == before
    for a in range(5):
        _same(eng.prediction_probability(ln[a], wd[a], agent=a), solo[a], a)


def test_refusals_leave_the_state_readable():
    from frenetix_motion_planner_amd import _abi
    small = [SHAPES[0], SHAPES[2], SHAPES[4]]
    # one agent of the batch evaluated select-only
    inps = [_make(small[0]), _make(small[1], write_bundle=False), _make(small[2])]
    with _engine(3) as eng:
        eng.plan_batch(inps)
        for a in (0, 2):
            _scene(eng, a, small[a])
        eng.set_risk_obstacles(_tables({}), 1)
        want = {a: eng.prediction_probability(EGO_L, EGO_W, agent=a) for a in (0, 2)}
        r = _raw(eng, [2, 1, 0])
        assert r[0] == _abi.FX_ERR_NOT_READY and "agent 1" in r[1] and "FX_MODE_WRITE_BUNDLE" in r[1] and _untouched(r)
        with pytest.raises(ValueError, match="agent 1"):
            eng.prediction_probability_batch(EGO_L, EGO_W)
        for a in (0, 2):
            _same(eng.prediction_probability(EGO_L, EGO_W, agent=a), want[a], a)
        for r, a in zip(eng.prediction_probability_batch(EGO_L, EGO_W, agents=[2, 0]), (2, 0)):
            _same(r, want[a], a)
    # a step without the cost map; a cost list without the prediction
    for kw, code, word in ((dict(write_costmap=False), _abi.FX_ERR_NOT_READY, "FX_MODE_WRITE_COSTMAP"),
                           (dict(cost_weights=dict(lateral_jerk=0.2, velocity_offset=1.0)), _abi.FX_ERR_INVALID_ARGUMENT, "FX_COST_PREDICTION")):
        inps = [_make(small[0]), _make(small[2], **kw)]
        with _engine(2) as eng:
            eng.plan_batch(inps)
            for a in range(2):
                eng.set_risk_obstacles(_tables({}), a)
            want = eng.prediction_probability(EGO_L, EGO_W, agent=0)
            before = eng.device_bytes
            r = _raw(eng, [0, 1])
            assert r[0] == code and "agent 1" in r[1] and word in r[1] and _untouched(r), r[:2]
            assert eng.device_bytes == before
            _same(eng.prediction_probability(EGO_L, EGO_W, agent=0), want, kw)
    # before the first evaluated step, and after update_state without an evaluation
    inps = [_make(small[0]), _make(small[2])]
    with _engine(2) as eng:
        assert _raw(eng, [])[0] == _abi.FX_OK
        eng._inputs = inps   # (for _raw's row count: nothing is uploaded yet)
        r = _raw(eng, [0, 1])
        assert r[0] == _abi.FX_ERR_NOT_READY and _untouched(r)
        eng._inputs = []
        eng.plan_batch(inps)
        for a in range(2):
            _scene(eng, a, small[2 * a])
        want = eng.prediction_probability_batch(EGO_L, EGO_W)
        eng.update_state(eng.make_state_update(v_des=inps[1].v_des + 1.0), agent=1)
        r = _raw(eng, [0, 1])
        assert r[0] == _abi.FX_ERR_NOT_READY and "rewritten" in r[1] and _untouched(r)
        eng.evaluate()
        eng.finish()
        again = eng.prediction_probability_batch(EGO_L, EGO_W)
        _same(again[0], want[0])                                    # (agent 0's inputs are what they were)
        _same(again[1], eng.prediction_probability(EGO_L, EGO_W, agent=1))
        assert not np.array_equal(again[1]["total"], want[1]["total"], equal_nan=True)   # (another desired velocity: other costs)


def test_memory():
    """a context that never calls the batched form reports the bytes it reports without it: nothing is allocated at creation, by a
    step or by the tables; the call takes its memory from the risk passes' one block, which a per-agent call behind it reuses"""
    inps = [_make(s) for s in SHAPES]
    seen = []
    for call in (False, True):
        with _engine() as eng:
            b0 = eng.device_bytes
            eng.plan_batch(inps)
            for a, s in enumerate(SHAPES):
                _scene(eng, a, s)
            b1 = eng.device_bytes
            seen.append((b0, b1))
            if not call:
                continue
            assert eng.last_predprob_ms == -1.0
            eng.prediction_probability_batch(EGO_L, EGO_W)
            b2 = eng.device_bytes
            # at least the scratch of the one round: [K][S - 1][whole tiles] doubles of agents 1 to 4
            assert b2 - b1 > 8 * (1 * 20 * 256 + 8 * 30 * 320 + 20 * 30 * 2176 + 5 * 30 * 64)
            eng.prediction_probability(EGO_L, EGO_W, agent=3)      # (its block is smaller than the batch's: no growth, no second block)
            eng.prediction_probability_batch(EGO_L, EGO_W, agents=[4, 2])
            assert eng.device_bytes == b2
    assert seen[0] == seen[1]
