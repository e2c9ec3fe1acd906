"""The plain risk pass over a whole agent batch in one call, with id lists or without (fx_eval_risk_batch),
against the per-agent call on the same context -- bit for bit, whichever agents and forms share a call, however the list positions
are cut into rounds and the steps into chunks -- and, independently of that shared code, against the NumPy restatement
(tests/risk_restatement.py) at the bound of tests/test_risk_gpu.py, 1e-12 relative to max(|want|, 1).

Shapes: those of tests/test_predprob_batch_gpu.py, the smallest at which the mapping of (agent, tile, chunk, obstacle, list
position) can go wrong; scenes as tests/test_resp_batch_gpu.py builds them:
  agent 0: (3, 5, 3)  =   60 candidates, K = 0          no item at all, every selected risk 0.0
  agent 1: (4, 8, 7)  =  256 candidates, K = 1, 2.0 s   S = 21: another chunk count
  agent 2: (5, 7, 8)  =  315 candidates, K = 8          a tile remainder
  agent 3: (8, 16, 16) = 2 176 candidates, K = 20, seed 7, some predictions S - 7 long, Mahalanobis
  agent 4: (2, 4, 4)  =   40 candidates, K = 5          less than a tile, ref_speed harm
Every agent has its own ego length, width and mass."""
import ctypes as C

import numpy as np
import pytest

from tests import risk_restatement as rr
from tests.test_predprob_batch_gpu import COUNTS, SHAPES, _engine, _make
from tests.test_resp_batch_gpu import MODES, REACH, _ego, _scene
from tests.test_risk_gpu import HARM

pytestmark = pytest.mark.gpu

NEED = 0xB   # VALID | FEASIBLE | RETURNED


def _same(got, want, what=""):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, what
    assert np.array_equal(got[0], want[0], equal_nan=True), (what, "ego_risk")
    assert np.array_equal(got[1], want[1], equal_nan=True), (what, "obst_risk")
    assert got[2] == want[2], (what, "min_risk_index", got[2], want[2])


def _lists(scenes):
    """the mixed forms of one call: none, one id (the winner), 65 descending ids with gaps (some without the flags), none, all 40"""
    ok1 = np.nonzero((scenes[1]["flags"] & NEED) == NEED)[0]
    f2 = scenes[2]["flags"]
    lack, good = np.nonzero((f2 & NEED) != NEED)[0][::5][:20], np.nonzero((f2 & NEED) == NEED)[0]
    good = good[::2] if len(good) >= 2 * (65 - len(lack)) else good
    l2 = np.sort(np.concatenate([lack, good[:65 - len(lack)]]))[::-1].copy()
    assert len(l2) == 65 and len(lack) > 0 and np.all(np.diff(l2) < 0) and (np.diff(l2) < -1).any()
    return [None, np.array([ok1[len(ok1) // 2]]), l2, None, np.arange(40)]


def _batch(eng, scenes, ids=None, agents=None):
    lst = list(range(len(scenes))) if agents is None else agents
    return eng.risk_batch([scenes[a]["params"] for a in lst], None if ids is None else [ids[a] for a in lst], agents=agents)


def _solo(eng, scenes, a, ids=None):
    return eng.risk(scenes[a]["params"], ids, agent=a)


@pytest.fixture(scope="module")
def ctx():
    """one context of five agents with their scenes, the per-agent calls of the mixed forms and the batched call -- computed once,
    left unchanged"""
    inps = [_make(s) for s in SHAPES]
    assert [i.n_candidates for i in inps] == COUNTS and [i.n_samples for i in inps] == [31, 21, 31, 31, 31]
    eng = _engine()
    eng.plan_batch(inps)
    scenes = [_scene(eng, a, s, inps[a], MODES[a], REACH[a]) for a, s in enumerate(SHAPES)]
    ids = _lists(scenes)
    solo = [_solo(eng, scenes, a, ids[a]) for a in range(5)]
    batch = _batch(eng, scenes, ids)
    yield eng, inps, scenes, ids, solo, batch
    eng.close()


def test_batch_equals_agents_alone(ctx):
    eng, inps, scenes, ids, solo, batch = ctx
    assert len(batch) == 5
    for a in range(5):
        _same(batch[a], solo[a], a)
        assert batch[a][0].shape == ((COUNTS[a],) if ids[a] is None else (len(ids[a]),))
    # agent 0: K = 0, no item, every selected risk 0.0 and NaN rows for the others; the arg-min is the first selected candidate
    f0 = scenes[0]["flags"]
    sel0 = (f0 & NEED) == NEED
    assert sel0.any() and np.all(batch[0][0][sel0] == 0.0) and np.all(batch[0][1][sel0] == 0.0)
    assert np.all(np.isnan(batch[0][0][~sel0])) and batch[0][2] == np.nonzero(sel0)[0][0]
    # agent 1: its one id
    assert batch[1][2] == ids[1][0] and not np.isnan(batch[1][0]).any()
    # agent 2: listed means evaluated, whatever the flags
    f2 = scenes[2]["flags"][ids[2]]
    lacking = int(((f2 & NEED) != NEED).sum())
    print(f"agent 2: {lacking} of 65 listed candidates lack a flag of VALID | FEASIBLE | RETURNED")
    with_flags = (f2 & NEED) == NEED
    assert lacking > 0 and not np.isnan(batch[2][0][with_flags]).any() and not np.isnan(batch[2][1][with_flags]).any()
    assert batch[2][2] in set(ids[2].tolist())    # agent 3: several chunks, NaN rows exactly for the unselected candidates, risks above zero
    from frenetix_motion_planner_amd._lib import lib
    cs3 = lib().fx_risk_items_chunk_steps(COUNTS[3], 31, 20)
    f3 = scenes[3]["flags"]
    sel3 = (f3 & NEED) == NEED
    print(f"agent 3: {cs3} steps per chunk, {int(sel3.sum())} of {COUNTS[3]} selected, {int((batch[3][0][sel3] > 0).sum())} with a risk")
    assert -(-30 // cs3) > 1 and (~sel3).any()
    assert np.all(np.isnan(batch[3][0][~sel3])) and not np.isnan(batch[3][0][sel3]).any()
    assert (batch[3][0][sel3] > 0).sum() > sel3.sum() // 4
    assert {len(p["pos_list"]) for p in scenes[3]["preds"].values()} == {30, 24}
    # agent 4: all 40 listed equals the values of its whole-candidate form where that one evaluates
    whole = _solo(eng, scenes, 4)
    sel4 = (scenes[4]["flags"] & NEED) == NEED
    assert np.array_equal(batch[4][0][sel4], whole[0][sel4]) and np.array_equal(batch[4][1][sel4], whole[1][sel4])
    assert (batch[4][0] > 0).any()
    # the views lie in the concatenated arrays at the sums of n_a of the agents in front
    n_a = [len(b[0]) for b in batch]
    assert n_a == [60, 1, 65, 2176, 40]
    off = np.concatenate([[0], np.cumsum(n_a)])
    for k in (0, 1):
        base = batch[0][k].base
        assert base is not None and all(b[k].base is base for b in batch)
        first = batch[0][k].__array_interface__["data"][0]
        assert [b[k].__array_interface__["data"][0] - first for b in batch] == [8 * int(o) for o in off[:-1]]
    assert eng.last_risk_ms > 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_tile_edges(ctx, n):
    """agent 3 listed with n ids (a stride that leaves the order ascending, then reversed) beside the others"""
    eng, inps, scenes, ids, solo, batch = ctx
    l3 = (np.arange(n) * 16 + 5)[::-1].copy()
    assert l3.max() < COUNTS[3]
    lists = list(ids)
    lists[3] = l3
    res = _batch(eng, scenes, lists)
    _same(res[3], _solo(eng, scenes, 3, l3), n)
    for a in (0, 1, 2, 4):
        _same(res[a], solo[a], (n, a))


def test_subsets_and_orders(ctx):
    eng, inps, scenes, ids, solo, batch = ctx
    for agents in ([3, 1], [4], [2, 0, 4]):
        res = _batch(eng, scenes, ids, agents)
        assert len(res) == len(agents)
        for r, a in zip(res, agents):
            _same(r, solo[a], (agents, a))
    # no agent has a list: the n_ids == NULL form
    for r, a in zip(_batch(eng, scenes, None, [4, 2]), (4, 2)):
        _same(r, _solo(eng, scenes, a), ("no lists", a))
    # one parameter object for all
    for r, a in zip(eng.risk_batch(scenes[2]["params"], [ids[2], ids[1]], agents=[2, 1]), (2, 1)):
        _same(r, eng.risk(scenes[2]["params"], ids[a], agent=a), ("one params", a))
    # an empty list is a list: no rows, no winner
    e = eng.risk_batch([scenes[1]["params"], scenes[4]["params"]], [np.zeros(0, np.int64), None], agents=[1, 4])
    assert e[0][0].shape == (0,) and e[0][2] == -1
    _same(e[1], _solo(eng, scenes, 4), "beside an empty list")


def test_chunks(ctx):
    """fx_risk_items_set_chunk_steps of 1, 7 and S - 1 against the automatic rule: the same bits"""
    from frenetix_motion_planner_amd._lib import lib
    eng, inps, scenes, ids, solo, batch = ctx
    L = lib()
    try:
        for cs in (1, 7, 30):      # (S - 1 of the four agents with S = 31; agent 1 is capped at its own 20)
            L.fx_risk_items_set_chunk_steps(cs)
            for a, r in enumerate(_batch(eng, scenes, ids)):
                _same(r, solo[a], (cs, a))
    finally:
        L.fx_risk_items_set_chunk_steps(0)
    for a, r in enumerate(_batch(eng, scenes, ids)):
        _same(r, batch[a], a)


def test_rounds(ctx):
    """a scratch limit under which the call takes at least three rounds and agent 3's candidates are cut at a tile boundary inside
    a round it shares with agent 2: the same bits.  One candidate's share of the scratch: 8 * 2 * K * chunks bytes"""
    from frenetix_motion_planner_amd._lib import lib
    eng, inps, scenes, ids, solo, batch = ctx
    L = lib()

    def share(n, S, K):
        return 8 * 2 * K * -(-(S - 1) // L.fx_risk_items_chunk_steps(n, S, K))

    s1, s2, s3, s4 = share(1, 21, 1), share(65, 31, 8), share(COUNTS[3], 31, 20), share(40, 31, 5)
    tile = lambda n: -(-n // 64) * 64
    # agent 1's tile, agent 2's two tiles and TWO tiles of agent 3 fit the first round; its other 32 tiles follow in rounds of
    # at most 12, so there are at least four rounds
    limit = tile(1) * s1 + tile(65) * s2 + 2 * 64 * s3 + 64 * s3 // 2
    rest = (COUNTS[3] // 64 - 2) * 64 * s3 + tile(40) * s4
    print(f"shares {s1}, {s2}, {s3}, {s4} bytes per candidate; limit {limit} bytes; at least {1 + -(-rest // limit)} rounds")
    assert limit < 12 * 64 * s3 + 64 * s3 and 1 + -(-rest // limit) >= 3
    try:
        for lim in (limit, 1 << 16, 1):
            L.fx_risk_batch_set_scratch_limit(lim)
            for a, r in enumerate(_batch(eng, scenes, ids)):
                _same(r, solo[a], (lim, a))
        L.fx_risk_items_set_chunk_steps(7)
        L.fx_risk_batch_set_scratch_limit(limit)
        for a, r in enumerate(_batch(eng, scenes, ids)):
            _same(r, solo[a], ("both", a))
    finally:
        L.fx_risk_items_set_chunk_steps(0)
        L.fx_risk_batch_set_scratch_limit(0)
    for a, r in enumerate(_batch(eng, scenes, ids)):
        _same(r, batch[a], a)


def test_ties_go_to_the_candidate_index(ctx):
    """agent 0 (K = 0: every risk 0.0) listed in descending order returns the SMALLEST listed candidate index, not ids[0]"""
    eng, inps, scenes, ids, solo, batch = ctx
    for l0 in (np.arange(59, 2, -3), np.array([17, 40, 3, 58])):
        lists = list(ids)
        lists[0] = l0
        res = _batch(eng, scenes, lists)
        assert np.all(res[0][0] == 0.0) and np.all(res[0][1] == 0.0)
        assert res[0][2] == l0.min() != l0[0]
        _same(res[0], _solo(eng, scenes, 0, l0))
        _same(res[3], solo[3])


def test_matches_the_restatement(ctx):
    """independent of the code the two calls share: agents 2 and 4 of ONE batched call (a list, the ref_speed harm) on the
    device's planes, at the bound and with the exclusions of tests/test_risk_gpu.py; the arg-min exact"""
    eng, inps, scenes, ids, solo, batch = ctx
    l2 = np.nonzero((scenes[2]["flags"] & NEED) == NEED)[0][::2]
    res = _batch(eng, scenes, [None, None, l2, None, None])
    for a, lst in ((2, l2), (4, np.nonzero((scenes[4]["flags"] & NEED) == NEED)[0])):
        sc = scenes[a]
        ego, obst, idx = res[a]
        if a == 4:
            ego, obst = ego[lst], obst[lst]
        P = [sc["planes"][n][lst] for n in ("x", "y", "theta", "v")]
        we, wo = rr.calc_risk(*P, sc["preds"], sc["typ"], MODES[a], HARM, **_ego(a))
        errs = [float((np.abs(g - w) / np.maximum(np.abs(w), 1.0)).max()) for g, w in ((ego, we), (obst, wo))]
        print(f"agent {a}: {len(lst)} candidates, {int((we > 0).sum())} with a risk, errors {errs[0]:.2e} / {errs[1]:.2e} (bound 1e-12)")
        assert (we > 0).sum() > len(lst) // 4, "too few candidates near an obstacle"
        assert max(errs) < 1e-12
        assert idx == rr.min_risk_index(ego, obst, lst)


def test_sparse_set_agent():
    """a context whose step ran select-only: after materialise(ids) a batch over that agent's ids equals the per-agent call; a
    batch naming an id outside the set is FX_ERR_NOT_READY, outputs untouched"""
    from frenetix_motion_planner_amd import _abi
    inps = [_make(SHAPES[2], write_bundle=False), _make(SHAPES[4])]
    with _engine(2) as eng, _engine(1) as full:
        eng.plan_batch(inps)
        full.plan_batch([_make(SHAPES[2])])
        sc_full = _scene(full, 0, SHAPES[2], inps[0])        # (the planes the obstacles walk along: a bundle-mode twin of agent 0)
        from frenetix_motion_planner_amd import risk
        eng.set_risk_obstacles(risk.obstacle_tables(sc_full["preds"], sc_full["typ"]), 0)
        scenes = [dict(sc_full, flags=eng.costs(0)[1]), _scene(eng, 1, SHAPES[4], inps[1])]
        ok = np.nonzero((scenes[0]["flags"] & NEED) == NEED)[0]
        sub = ok[np.arange(len(ok)) % 3 != 1][:70]
        assert len(sub) > 64      # (more than a tile)
        eng.materialise(sub, agent=0)
        order = sub[::-1].copy()
        want = [_solo(eng, scenes, 0, order), _solo(eng, scenes, 1)]
        got = _batch(eng, scenes, [order, None])
        _same(got[0], want[0], "sparse"), _same(got[1], want[1], "beside the sparse one")
        assert got[0][2] in set(sub.tolist()) and (got[0][0] > 0).any()
        outside = np.setdiff1d(ok, sub)[:1]
        bad = np.concatenate([order[:5], outside])
        r = _raw(eng, [1, 0], scenes, [None, bad])
        assert r[0] == _abi.FX_ERR_NOT_READY and "agent 0" in r[1] and "FX_MODE_WRITE_BUNDLE" in r[1] and _untouched(r), r[:2]
        r = _raw(eng, [1, 0], scenes, [None, None])      # (without a list a step without a bundle has nothing to read)
        assert r[0] == _abi.FX_ERR_NOT_READY and "agent 0" in r[1] and _untouched(r), r[:2]
        _same(_batch(eng, scenes, [order, None])[0], want[0], "after the refusals")


def test_nothing_else_moves(ctx):
    from frenetix_motion_planner_amd import risk
    eng, inps, scenes, ids, solo, batch = ctx

    def state():
        # (the result block but for the device times it reports, which depend on when it is read)
        block = [{k: repr(v) for k, v in r.items() if "ms" not in k and "time" not in k} for r in eng.finish()]
        return [eng.costs(a) for a in range(5)], eng.step_info(), block

    cp =risk.risk_cost_params([1, 1, 1, 1, 1], responsibility=scenes[3]["vec"])
    rc0 = eng.risk_costs(scenes[3]["params"], cp, agent=3)
    rb0 = eng.responsibility_cost_batch([scenes[a]["params"] for a in (3, 2)], [scenes[a]["cost"] for a in (3, 2)],
                                        [scenes[a]["weight"] for a in (3, 2)], agents=[3, 2])
    s0 = state()
    bytes0 = eng.device_bytes
    got = _batch(eng, scenes, ids)
    assert eng.device_bytes >= bytes0
    s1 = state()
    for (c0, f0), (c1, f1) in zip(s0[0], s1[0]):
        assert np.array_equal(c0, c1, equal_nan=True) and np.array_equal(f0, f1)
    assert s0[1] == s1[1] and s0[2] == s1[2] and len(s0[2]) == 5 and "best_index" in s0[2][0]
    for a in range(5):
        _same(got[a], solo[a], a)
        _same(_solo(eng, scenes, a, ids[a]), solo[a], ("per-agent after the batch", a))
    rc1 = eng.risk_costs(scenes[3]["params"], cp, agent=3)
    for k, v in rc0.items():
        assert np.array_equal(v, rc1[k], equal_nan=True), k
    rb1 = eng.responsibility_cost_batch([scenes[a]["params"] for a in (3, 2)], [scenes[a]["cost"] for a in (3, 2)],
                                        [scenes[a]["weight"] for a in (3, 2)], agents=[3, 2])
    for r0, r1 in zip(rb0, rb1):
        for k in ("resp", "total", "ego_risk", "obst_risk"):
            assert np.array_equal(r0[k], r1[k], equal_nan=True), k
        assert r0["best_index"] == r1["best_index"]
    # the risk of the responsibility pass (costed candidates) and of this pass (VALID | FEASIBLE | RETURNED) agree where both evaluate
    both = ~np.isnan(rb1[0]["ego_risk"]) & ~np.isnan(solo[3][0])
    assert both.sum() > 100 and np.array_equal(rb1[0]["ego_risk"][both], solo[3][0][both])
    b2 = eng.device_bytes
    _batch(eng, scenes, ids)
    assert eng.device_bytes == b2 >= bytes0


def _raw(eng, agents, scenes, lists, n=None, null=None, params_null=False):
    """the library's call with outputs filled with 7: (status, message, the three output arrays); lists[i]: None or ids, or the
    pair (n_ids, None) for a count without a list"""
    from frenetix_motion_planner_amd import _abi
    from frenetix_motion_planner_amd._lib import lib
    n = len(agents) if n is None else n
    m = max(len(agents), 1)
    pi64 = C.POINTER(C.c_int64)
    rows = 0
    keep, cnt, ptr = [], [], []
    for a, x in zip(agents, lists):
        if isinstance(x, tuple):
            cnt.append(x[0]), ptr.append(C.cast(None, pi64))
            continue
        if x is None:
            rows += eng._inputs[a].n_candidates if 0 <= a < len(eng._inputs) else 0
            cnt.append(0), ptr.append(C.cast(None, pi64))
        else:
            x = np.ascontiguousarray(x, np.int64)
            keep.append(x)
            rows += len(x)
            cnt.append(len(x)), ptr.append(x.ctypes.data_as(pi64))
    arr = [np.full(max(rows, 1), 7.0), np.full(max(rows, 1), 7.0), np.full(m, 7, np.int64)]
    sc = [scenes[a if 0 <= a < len(scenes) else 0] for a in agents]
    params = (_abi.FxRiskParams * m)(*[s["params"] for s in sc])
    out = _abi.FxRiskBatchOutputs(*[None if null == k else x.ctypes.data for k, x in enumerate(arr)])
    al = np.ascontiguousarray(agents, np.int32)
    n_ids = np.asarray(cnt + [0], np.int64)
    rc = lib().fx_eval_risk_batch(eng._ctx, n, al.ctypes.data_as(C.POINTER(C.c_int32)), None if params_null else params,
                                  n_ids.ctypes.data_as(pi64), (pi64 * m)(*ptr), C.byref(out))
    return rc, lib().fx_last_error().decode(), arr


def _untouched(r):
    return all(np.all(x == 7) for x in r[2])


def test_refusals(ctx):
    from frenetix_motion_planner_amd import _abi
    eng, inps, scenes, ids, solo, batch = ctx
    before = eng.device_bytes
    INV = _abi.FX_ERR_INVALID_ARGUMENT
    cases = (("duplicate", _raw(eng, [1, 2, 1], scenes, [ids[1], ids[2], None]), "agent 1 listed twice"),
             ("out of range", _raw(eng, [0, 5], scenes, [None, None]), "agent 5"),
             ("negative", _raw(eng, [0, -1], scenes, [None, None]), "agent -1"),
             ("too many", _raw(eng, [0, 1, 2, 3, 4, 4], scenes, [None] * 6, n=6), "n_agents 6"),
             ("negative count", _raw(eng, [0], scenes, [None], n=-1), "n_agents -1"),
             ("id out of range", _raw(eng, [3, 2, 4], scenes, [None, np.array([5, COUNTS[2], 7]), None]), "agent 2"),
             ("negative id", _raw(eng, [4, 1], scenes, [np.array([3, -1]), None]), "agent 4"),
             ("a count without a list", _raw(eng, [2, 3], scenes, [ids[2], (4, None)]), "agent 3"),
             ("NULL output", _raw(eng, [1, 2], scenes, [ids[1], ids[2]], null=2), "output pointer"),
             ("NULL params", _raw(eng, [1, 2], scenes, [ids[1], ids[2]], params_null=True), "params"))
    for name, r, word in cases:
        assert r[0] == INV and word in r[1] and _untouched(r), (name, r[:2])
    assert str(COUNTS[2]) in cases[5][1][1]
    r = _raw(eng, [0, 1], scenes, [None, None], n=0)
    assert r[0] == _abi.FX_OK and _untouched(r)
    with pytest.raises(ValueError, match="agent 2"):
        eng.risk_batch([scenes[a]["params"] for a in (3, 2)], [None, [COUNTS[2]]], agents=[3, 2])
    with pytest.raises(ValueError):
        eng.risk_batch([scenes[0]["params"]], None, agents=[0, 1])
    assert eng.device_bytes == before
    for a, r in enumerate(_batch(eng, scenes, ids)):     # the pass still answers, and the same
        _same(r, solo[a], a)


def test_a_stale_step_is_refused():
    """fx_update_state without an evaluation: NOT_READY naming the agent, outputs untouched; the next evaluation makes it answer"""
    from frenetix_motion_planner_amd import _abi
    small = [SHAPES[0], SHAPES[4]]
    inps = [_make(s) for s in small]
    with _engine(2) as eng:
        eng._inputs = inps   # (for _raw's row count: nothing is uploaded yet)
        dummy = [dict(params=_params(a)) for a in range(2)]
        r = _raw(eng, [0, 1], dummy, [None, None])
        assert r[0] == _abi.FX_ERR_NOT_READY and "agent 0" in r[1] and _untouched(r), r[:2]
        eng._inputs = []
        eng.plan_batch(inps)
        scenes = [_scene(eng, a, small[a], inps[a]) for a in range(2)]
        lists = [np.array([7, 3]), None]
        want = _batch(eng, scenes, lists)
        eng.update_state(eng.make_state_update(v_des=inps[1].v_des + 1.0), agent=1)
        r = _raw(eng, [1, 0], scenes, [None, lists[0]])
        assert r[0] == _abi.FX_ERR_NOT_READY and "rewritten" in r[1] and "agent 1" in r[1] and _untouched(r), r[:2]
        eng.evaluate()
        eng.finish()
        again = _batch(eng, scenes, lists)
        _same(again[0], want[0], "agent 0's inputs are what they were")
        _same(again[1], _solo(eng, scenes, 1), "agent 1 after its new step")


def _params(a):
    from frenetix_motion_planner_amd import risk
    return risk.risk_params(MODES[0], HARM, **_ego(a))
