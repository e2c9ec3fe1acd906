"""The responsibility pass over a whole agent batch in one call (fx_eval_responsibility_cost_batch) against the
per-agent call on the same context -- bit for bit, whichever agents share a call, however the candidates are cut into rounds and the
steps into chunks -- and, independently of that shared code, against the NumPy restatement (tests/risk_costs_restatement.py) at the
bound of tests/test_responsibility_cost_gpu.py, (2 K + 1) 1e-12.

Shapes: those of tests/test_predprob_batch_gpu.py, the smallest at which the mapping of (agent, tile, chunk, obstacle) can go wrong:
  agent 0: (3, 5, 3)  =   60 candidates, K = 0          one partial tile and no item at all          reach-set mode
  agent 1: (4, 8, 7)  =  256 candidates, K = 1, 2.0 s   exact tiles, S = 21: another chunk count      action space
  agent 2: (5, 7, 8)  =  315 candidates, K = 8          a tile remainder                             reach-set mode
  agent 3: (8, 16, 16) = 2 176 candidates, K = 20, seed 7, some predictions S - 7 long               action space, Mahalanobis
  agent 4: (2, 4, 4)  =   40 candidates, K = 5          less than a tile                             reach-set mode, ref_speed harm
Every agent has its own ego length, width and mass and its own weight."""
import ctypes as C

import numpy as np
import pytest

from tests import predprob_restatement as pp
from tests import risk_costs_restatement as rcr
from tests.test_predprob_batch_gpu import COUNTS, SHAPES, _engine, _make
from tests.test_responsibility_cost_gpu import _resum
from tests.test_risk_costs_gpu import _err, _reach_sets
from tests.test_risk_gpu import BASE, HARM, _predictions

pytestmark = pytest.mark.gpu

COSTED, NEED = 0x10, 0xB
KEYS = ("resp", "total", "ego_risk", "obst_risk")
from tests.risk_scenes import MODES  # noqa: E402
REACH = [True, False, True, False, True]


from tests.risk_scenes import ego as _ego, resp_cost as _cost, weight as _weight  # noqa: E402,F401


def _scene(eng, a, shape, inp, modes=BASE, reach=True):
    """agent a's K obstacles along its own candidates, reach sets on the first ones and the action-space vector, set on the engine;
    what the calls and the restatement need of it"""
    from frenetix_motion_planner_amd import risk
    _, flags = eng.costs(a)
    planes = {n: eng.plane(n, a).T.copy() for n in ("x", "y", "theta", "v")}
    K = shape["K"]
    maha = bool(modes.get("fast_prob_mahalanobis"))
    preds, typ = _predictions(planes, flags, np.random.default_rng(shape["seed"]), n_obs=K, zero_cov=not maha) if K else ({}, {})
    keys = list(preds)
    ok = np.nonzero((flags & NEED) == NEED)[0]
    x0 = np.array([planes["x"][ok[0], 0], planes["y"][ok[0], 0]])
    th0 = float(planes["theta"][ok[0], 0]) + 0.5
    # (the synthetic sets reach step 21: none for the agent whose horizon ends at step 20, which runs in action-space mode)
    sets = _reach_sets(planes, keys, ok[::3], inp.dt) if K and inp.n_samples > 22 else {}
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ, mahalanobis=maha), a)
    eng.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples), a)
    vec = risk.action_space_responsibility(preds, x0, th0)
    return dict(flags=flags, planes=planes, preds=preds, typ=typ, keys=keys, sets=sets, vec=vec, x0=x0, th0=th0, modes=modes,
                params=risk.risk_params(modes, HARM, **_ego(a)), cost=_cost("reach_set" if reach else vec), weight=_weight(a))


def _same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)
    assert got["best_index"] == want["best_index"], what
    assert np.array_equal(np.float64(got["best_cost"]).view(np.uint64), np.float64(want["best_cost"]).view(np.uint64)), what


def _batch(eng, scenes, agents=None, **kw):
    lst = list(range(len(scenes))) if agents is None else agents
    return eng.responsibility_cost_batch([scenes[a]["params"] for a in lst], [scenes[a]["cost"] for a in lst],
                                         [scenes[a]["weight"] for a in lst], agents=agents, **kw)


def _solo(eng, scenes, a, **kw):
    s = scenes[a]
    return eng.responsibility_cost(s["params"], s["cost"], s["weight"], agent=a, **kw)


@pytest.fixture(scope="module")
def ctx():
    """one context of five agents with their scenes, the per-agent calls and the batched call -- computed once, left unchanged"""
    inps = [_make(s) for s in SHAPES]
    assert [i.n_candidates for i in inps] == COUNTS and [i.n_samples for i in inps] == [31, 21, 31, 31, 31]
    eng = _engine()
    eng.plan_batch(inps)
    scenes = [_scene(eng, a, s, inps[a], MODES[a], REACH[a]) for a, s in enumerate(SHAPES)]
    solo = [_solo(eng, scenes, a) for a in range(5)]
    batch = _batch(eng, scenes)
    yield eng, inps, scenes, solo, batch
    eng.close()


def test_batch_equals_agents_alone(ctx):
    eng, inps, scenes, solo, batch = ctx
    assert len(batch) == 5
    for a, (shape, sc) in enumerate(zip(SHAPES, scenes)):
        K, flags = shape["K"], sc["flags"]
        _same(batch[a], solo[a], a)
        assert batch[a]["prediction"] is None and all(batch[a][k].shape == (COUNTS[a],) for k in KEYS)
        ids = np.nonzero(flags & COSTED)[0]
        rest = np.setdiff1d(np.arange(COUNTS[a]), ids)
        assert len(ids) > 0
        for k in KEYS:
            assert np.all(np.isnan(batch[a][k][rest])) and not np.isnan(batch[a][k][ids]).any(), (a, k)
        assert batch[a]["best_index"] == pp.best_index(batch[a]["total"], flags), a
        nz = int((batch[a]["resp"][ids] != 0).sum())
        print(f"agent {a}: C = {COUNTS[a]}, S = {inps[a].n_samples}, K = {K}, {len(ids)} costed, {nz} with a responsibility cost")
        if K == 0:
            cost, _ = eng.costs(a)
            assert np.all(batch[a]["resp"][ids] == 0.0) and np.array_equal(batch[a]["total"][ids], cost[ids])
        if K >= 5:
            assert nz > len(ids) // 4, a
        if a == 3:
            assert {len(p["pos_list"]) for p in sc["preds"].values()} == {inps[a].n_samples - 1, inps[a].n_samples - 7}


@pytest.mark.parametrize("mode", ["reach", "action"])
def test_agent_2_matches_the_restatement(ctx, mode):
    """independent of the code the two calls share: agent 2's resp on its read-back planes, in both modes"""
    eng, inps, scenes, solo, batch = ctx
    a, sc = 2, scenes[2]
    K = SHAPES[a]["K"]
    sel = dict(scenes[a], cost=_cost("reach_set" if mode == "reach" else sc["vec"]))
    got = _batch(eng, {a: sel}, agents=[a])[0] if mode == "action" else batch[a]
    ids = np.nonzero(sc["flags"] & COSTED)[0]
    P = [sc["planes"][n][ids] for n in ("x", "y", "theta", "v")]
    want = rcr.calc_risk_detail(*P, sc["preds"], sc["typ"], BASE, HARM, **_ego(a))
    if mode == "action":
        wr = [rcr.responsibility_action_space(want["obst_risk_max"][c], sc["preds"], sc["x0"], sc["th0"]) for c in range(len(ids))]
    else:
        wr = [rcr.responsibility_reach_set(P[0][c], P[1][c], inps[a].dt, sc["sets"], want["obst_risk_max"][c], sc["keys"])[0]
              for c in range(len(ids))]
    wr = np.asarray(wr, np.float64)
    err = _err(got["resp"][ids], wr)
    print(f"{mode}: resp {err:.2e} (bound {(2 * K + 1) * 1e-12:.1e}); {int((wr != 0).sum())} of {len(ids)} candidates with a cost")
    assert (wr != 0).sum() > len(ids) // 8
    assert err < (2 * K + 1) * 1e-12


def test_subsets_and_order(ctx):
    eng, inps, scenes, solo, batch = ctx
    for agents in ([3, 1], [2], [4, 0, 3], None):
        lst = list(range(5)) if agents is None else agents
        res = _batch(eng, scenes, agents)
        assert len(res) == len(lst)
        for r, a in zip(res, lst):
            _same(r, solo[a], (agents, a))
        # the views lie in the concatenated arrays at the sums of C of the agents in front
        off = np.concatenate([[0], np.cumsum([COUNTS[a] for a in lst])])
        for k in KEYS:
            base = res[0][k].base
            assert base is not None and all(r[k].base is base for r in res)
            first = res[0][k].__array_interface__["data"][0]
            assert [r[k].__array_interface__["data"][0] - first for r in res] == [8 * int(o) for o in off[:-1]]


def test_partition_independence(ctx):
    """other rounds, other chunks, the same bits.  Scratch per candidate at the automatic chunk size: 56 K chunks bytes"""
    from frenetix_motion_planner_amd._lib import lib
    eng, inps, scenes, solo, batch = ctx
    L = lib()
    cs2 = L.fx_risk_items_chunk_steps(COUNTS[2], 31, 8)
    share2 = 56 * 8 * -(-30 // cs2)
    try:
        for limit in (3 * 64 * share2, 1 << 20, 1):
            L.fx_risk_batch_set_scratch_limit(limit)
            for a, r in enumerate(_batch(eng, scenes)):
                _same(r, solo[a], (limit, a))
        L.fx_risk_batch_set_scratch_limit(0)
        for cs in (1, 7, 30):      # (S - 1 of the four agents with S = 31; agent 1 is capped at its own 20)
            L.fx_risk_items_set_chunk_steps(cs)
            for a, r in enumerate(_batch(eng, scenes)):
                _same(r, solo[a], (cs, a))
        L.fx_risk_items_set_chunk_steps(7)
        L.fx_risk_batch_set_scratch_limit(1 << 20)
        for a, r in enumerate(_batch(eng, scenes)):
            _same(r, solo[a], ("both", a))
    finally:
        L.fx_risk_items_set_chunk_steps(0)
        L.fx_risk_batch_set_scratch_limit(0)
    one, two = _batch(eng, scenes), _batch(eng, scenes)
    for a in range(5):
        _same(one[a], two[a], a)
        _same(one[a], batch[a], a)
    assert eng.last_risk_ms > 0


def test_prediction_probability(ctx):
    eng, inps, scenes, solo, batch = ctx
    res = _batch(eng, scenes, prediction="probability")
    prob = eng.prediction_probability_batch([_ego(a)["ego_length"] for a in range(5)], [_ego(a)["ego_width"] for a in range(5)])
    moved = 0
    for a in range(5):
        want = _solo(eng, scenes, a, prediction="probability")
        _same(res[a], want, a)
        assert np.array_equal(res[a]["prediction"], prob[a]["prob"], equal_nan=True)
        assert np.array_equal(res[a]["prediction"], want["prediction"], equal_nan=True)
        moved += not np.array_equal(res[a]["total"], batch[a]["total"], equal_nan=True)
    assert moved >= 3
    # a word per agent: the probability for some, the step's own entry for the others
    mixed = _batch(eng, scenes, agents=[3, 2, 4], prediction=["probability", "step", "probability"])
    _same(mixed[0], res[3]), _same(mixed[1], batch[2]), _same(mixed[2], res[4])
    assert mixed[1]["prediction"] is None and np.array_equal(mixed[2]["prediction"], prob[4]["prob"], equal_nan=True)


@pytest.mark.parametrize("case", ["split", "fused"])
def test_total_is_the_resum_on_both_kinds_of_step(case):
    inps = [_make(s) for s in SHAPES[1:4]]
    with _engine(3) as eng:
        eng.set_obstacle_stage(2 if case == "split" else 1)
        eng.plan_batch(inps)
        info = eng.step_info()
        deferred = bool(info["obstacle_kernel"])
        assert deferred == (case == "split")
        scenes = [_scene(eng, a, s, inps[a], BASE, a % 2 == 1) for a, s in enumerate(SHAPES[1:4])]
        res = _batch(eng, scenes)
        for a, r in enumerate(res):
            sel = np.nonzero(scenes[a]["flags"] & COSTED)[0]
            names, w = list(inps[a].cost_names), np.asarray(inps[a]._cost_w, np.float64)
            raw = eng.costmap(a)
            assert len(sel) > 30 and "prediction" in names
            assert np.array_equal(r["total"][sel], _resum(raw[sel], w, names, scenes[a]["weight"], r["resp"][sel], deferred)), (case, a)
            _same(r, _solo(eng, scenes, a), (case, a))
        assert (res[2]["resp"][np.nonzero(scenes[2]["flags"] & COSTED)[0]] != 0).any()


def test_33_agents():
    """one agent of 2 176 candidates and 32 of 40 to 315: more rows than half a wave looks up at once, and no fixed-size table"""
    small = [SHAPES[0], SHAPES[2], SHAPES[4]]
    shapes = [small[a % 3] for a in range(20)] + [SHAPES[3]] + [small[a % 3] for a in range(12)]
    inps = [_make(s, v0=8.0 + 0.1 * a) for a, s in enumerate(shapes)]
    with _engine() as eng:
        eng.plan_batch(inps)
        scenes = [_scene(eng, a, dict(s, K=3 if a != 20 else 20), inps[a], BASE, a % 2 == 0) for a, s in enumerate(shapes)]
        res = _batch(eng, scenes)
        some = _batch(eng, scenes, agents=[32, 20, 0])
        assert len(res) == 33
        nz = 0
        for a in range(33):
            want = _solo(eng, scenes, a)
            _same(res[a], want, a)
            nz += int(np.nansum(want["resp"] != 0) > 0)
        print(f"{nz} of 33 agents with a responsibility cost")
        assert np.nansum(res[20]["resp"] != 0) > 0 and nz > 16
        for r, a in zip(some, (32, 20, 0)):
            _same(r, res[a], a)


def _raw(eng, agents, scenes, n=None, weights=None, modes=None, null=None):
    """the library's call with outputs filled with 7.0: (status, message, the six output arrays)"""
    from frenetix_motion_planner_amd import _abi
    from frenetix_motion_planner_amd._lib import lib
    n = len(agents) if n is None else n
    m = max(len(agents), 1)
    rows = sum(eng._inputs[a].n_candidates for a in agents if 0 <= a < len(eng._inputs))
    arr = [np.full(max(rows, 1), 7.0) for _ in range(4)] + [np.full(m, 7, np.int64), np.full(m, 7.0)]
    sc = [scenes[a if 0 <= a < len(scenes) else 0] for a in agents]
    params = (_abi.FxRiskParams * m)(*[s["params"] for s in sc])
    rps = (_abi.FxRespCostParams * m)(*[
        _abi.FxRespCostParams(float(s["weight"] if weights is None else weights[i]),
                              int(s["cost"].responsibility_mode if modes is None else modes[i]), s["cost"].responsibility, None)
        for i, s in enumerate(sc)])
    out = _abi.FxRespCostBatchOutputs(*[None if null == k else x.ctypes.data for k, x in enumerate(arr)])
    ids = np.ascontiguousarray(agents, np.int32)
    rc = lib().fx_eval_responsibility_cost_batch(eng._ctx, n, ids.ctypes.data_as(C.POINTER(C.c_int32)), params, rps, C.byref(out))
    return rc, lib().fx_last_error().decode(), arr


def _raw_agent(eng, a, s, weight=None, mode=None, null=False):
    """the per-agent call's status for the same agent and parameters"""
    from frenetix_motion_planner_amd import _abi
    from frenetix_motion_planner_amd._lib import lib
    n = max(eng._inputs[a].n_candidates, 1) if 0 <= a < len(eng._inputs) else 1
    arr = [np.zeros(n) for _ in range(4)] + [np.zeros(1, np.int64), np.zeros(1)]
    rp = _abi.FxRespCostParams(float(s["weight"] if weight is None else weight),
                               int(s["cost"].responsibility_mode if mode is None else mode), s["cost"].responsibility, None)
    out = _abi.FxRespCostOutputs(*[None if (null and k == 1) else x.ctypes.data for k, x in enumerate(arr)])
    return lib().fx_eval_responsibility_cost_agent(eng._ctx, a, C.byref(s["params"]), C.byref(rp), 0, None, C.byref(out))


def _untouched(r):
    return all(np.all(x == 7) for x in r[2])


def test_refusals_on_the_shared_context(ctx):
    from frenetix_motion_planner_amd import _abi, risk
    eng, inps, scenes, solo, batch = ctx
    before = eng.device_bytes
    INV = _abi.FX_ERR_INVALID_ARGUMENT
    nan = float("nan")
    cases = (("duplicate", _raw(eng, [1, 2, 1], scenes), "agent 1 listed twice", INV),
             ("out of range", _raw(eng, [0, 5], scenes), "agent 5", _raw_agent(eng, 5, scenes[0])),
             ("negative", _raw(eng, [0, -1], scenes), "agent -1", _raw_agent(eng, -1, scenes[0])),
             ("too many", _raw(eng, [0, 1, 2, 3, 4, 4], scenes, n=6), "", INV),
             ("zero weight", _raw(eng, [2, 3], scenes, weights=[0.5, 0.0]), "agent 3", _raw_agent(eng, 3, scenes[3], weight=0.0)),
             ("NaN weight", _raw(eng, [4, 1, 2], scenes, weights=[0.5, nan, 0.5]), "agent 1", _raw_agent(eng, 1, scenes[1], weight=nan)),
             ("unknown mode", _raw(eng, [2, 3], scenes, modes=[9, 1]), "agent 2", _raw_agent(eng, 2, scenes[2], mode=9)),
             ("no mode", _raw(eng, [3, 2], scenes, modes=[1, 0]), "agent 2", _raw_agent(eng, 2, scenes[2], mode=0)),
             ("NULL output", _raw(eng, [1, 2], scenes, null=1), "agent 1", _raw_agent(eng, 1, scenes[1], null=True)))
    for name, r, word, code in cases:
        assert r[0] == code == INV and word in r[1] and _untouched(r), (name, r[:2], code)
    r = _raw(eng, [0, 1], scenes, n=0)
    assert r[0] == _abi.FX_OK and _untouched(r)
    # an obstacle the detail pass cannot evaluate (np.max of an empty list upstream), at one agent
    sc = scenes[4]
    short = dict(sc["preds"])
    k1 = sc["keys"][1]
    short[k1] = dict(short[k1], pos_list=np.zeros((0, 2)), cov_list=np.zeros((0, 2, 2)), orientation_list=np.zeros(0), v_list=np.zeros(0))
    eng.set_risk_obstacles(risk.obstacle_tables(short, sc["typ"]), 4)
    r = _raw(eng, [2, 4, 3], scenes)
    assert r[0] == _raw_agent(eng, 4, sc) == INV and "agent 4" in r[1] and "obstacle 1" in r[1] and _untouched(r), r[:2]
    with pytest.raises(ValueError, match="agent 4"):
        _batch(eng, scenes)
    eng.set_risk_obstacles(risk.obstacle_tables(sc["preds"], sc["typ"]), 4)
    eng.set_reach_sets(risk.reach_set_tables(sc["sets"], sc["keys"], inps[4].dt, inps[4].n_samples), 4)
    # the Python-side refusals, per agent, before any call
    with pytest.raises(ValueError, match="agent 3"):
        eng.responsibility_cost_batch([scenes[a]["params"] for a in (2, 3)], [scenes[a]["cost"] for a in (2, 3)], [0.5, 0.0], agents=[2, 3])
    with pytest.raises(ValueError, match="agent 1"):
        eng.responsibility_cost_batch([scenes[a]["params"] for a in (1, 2)], [_cost(scenes[1]["vec"][:0]), scenes[2]["cost"]], [0.5, 0.5],
                                      agents=[1, 2])
    with pytest.raises(ValueError):
        _batch(eng, scenes, prediction="other")
    assert eng.device_bytes == before
    for a in range(5):     # the previous results are still readable, and the same
        _same(_solo(eng, scenes, a), solo[a], a)
    for a, r in enumerate(_batch(eng, scenes)):
        _same(r, solo[a], a)


def test_refusals_leave_the_state_readable():
    from frenetix_motion_planner_amd import _abi, risk
    small = [SHAPES[0], SHAPES[2], SHAPES[4]]
    # an agent of the batch without the bundle, without the cost map
    for kw, word in ((dict(write_bundle=False), "FX_MODE_WRITE_BUNDLE"), (dict(write_costmap=False), "FX_MODE_WRITE_COSTMAP")):
        inps = [_make(small[0]), _make(small[1], **kw), _make(small[2])]
        with _engine(3) as eng:
            eng.plan_batch(inps)
            scenes = {a: _scene(eng, a, small[a], inps[a]) for a in (0, 2)}
            scenes[1] = dict(scenes[2], cost=_cost("reach_set"))
            eng.set_risk_obstacles(risk.obstacle_tables({}, {}), 1)
            want = {a: _solo(eng, scenes, a) for a in (0, 2)}
            before = eng.device_bytes
            r = _raw(eng, [2, 1, 0], scenes)
            assert r[0] == _raw_agent(eng, 1, scenes[1]) == _abi.FX_ERR_NOT_READY and "agent 1" in r[1] and word in r[1] and _untouched(r), r[:2]
            with pytest.raises(ValueError, match="agent 1"):
                _batch(eng, scenes, agents=[0, 1, 2])
            assert eng.device_bytes == before
            for a in (0, 2):
                _same(_solo(eng, scenes, a), want[a], a)
            for r, a in zip(_batch(eng, scenes, agents=[2, 0]), (2, 0)):
                _same(r, want[a], a)
    # before the first evaluated step, and after update_state without an evaluation
    inps = [_make(small[0]), _make(small[2])]
    with _engine(2) as eng, _engine(2) as other:
        other.plan_batch(inps)
        scenes = [_scene(other, a, small[2 * a], inps[a]) for a in range(2)]   # (parameters of the right shapes; `eng` has no step yet)
        eng._inputs = inps   # (for _raw's row count: nothing is uploaded yet)
        r = _raw(eng, [0, 1], scenes)
        assert r[0] == _raw_agent(eng, 0, scenes[0]) == _abi.FX_ERR_NOT_READY and "agent 0" in r[1] and _untouched(r)
        eng._inputs = []
        eng.plan_batch(inps)
        scenes = [_scene(eng, a, small[2 * a], inps[a]) for a in range(2)]
        want = _batch(eng, scenes)
        eng.update_state(eng.make_state_update(v_des=inps[1].v_des + 1.0), agent=1)
        r = _raw(eng, [0, 1], scenes)
        assert r[0] == _raw_agent(eng, 0, scenes[0]) == _abi.FX_ERR_NOT_READY and "rewritten" in r[1] and "agent 0" in r[1] and _untouched(r)
        eng.evaluate()
        eng.finish()
        again = _batch(eng, scenes)
        _same(again[0], want[0])                                    # (agent 0's inputs are what they were)
        _same(again[1], _solo(eng, scenes, 1))
        assert not np.array_equal(again[1]["total"], want[1]["total"], equal_nan=True)   # (another desired velocity: other costs)


def test_memory():
    """a context that never makes the batched call reports the bytes it reports without it: nothing is allocated at creation, by a
    step or by the tables; the call takes its memory from the risk passes' one block, which grows on the first call and not on a
    second equal one"""
    from frenetix_motion_planner_amd._lib import lib
    inps = [_make(s) for s in SHAPES]
    seen = []
    for call in (False, True):
        with _engine() as eng:
            b0 = eng.device_bytes
            eng.plan_batch(inps)
            scenes = [_scene(eng, a, s, inps[a], MODES[a], REACH[a]) for a, s in enumerate(SHAPES)]
            b1 = eng.device_bytes
            seen.append((b0, b1))
            if not call:
                continue
            _batch(eng, scenes)
            b2 = eng.device_bytes
            # at least the partials of the one round, [K][chunks][7][whole tiles], and the columns [4][K][C], of agents 1 to 4
            part = sum(7 * K * -(-(S - 1) // lib().fx_risk_items_chunk_steps(n, S, K)) * -(-n // 64) * 64
                       for n, S, K in ((256, 21, 1), (315, 31, 8), (2176, 31, 20), (40, 31, 5)))
            col = sum(4 * K * n for n, K in ((256, 1), (315, 8), (2176, 20), (40, 5)))
            assert b2 - b1 > 8 * (part + col)
            _batch(eng, scenes)
            assert eng.device_bytes == b2
            _solo(eng, scenes, 3)                  # (its block is smaller than the batch's: no growth, no second block)
            _batch(eng, scenes, agents=[4, 2])
            assert eng.device_bytes == b2
    assert seen[0] == seen[1]
