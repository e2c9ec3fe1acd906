"""Risk detail and risk costs of a whole agent batch in one call, each agent with an id list or none and with cost parameters or
none (fx_eval_risk_costs_batch), against the per-agent call on the same context -- bit for bit (int64 views,
NaNs included), whichever agents and forms share a call, however the list positions are cut into rounds and the steps into chunks
-- and, independently of that shared code, against the NumPy restatement (tests/risk_costs_restatement.py over
tests/risk_restatement.py) at the bounds tests/test_risk_costs_gpu.py holds the per-agent call to.

Shapes and scenes: those of tests/test_predprob_batch_gpu.py / tests/test_resp_batch_gpu.py (see tests/test_risk_batch_gpu.py).  The
mixed forms of the shared call:
  agent 0:    60 candidates, K = 0          no list, detail only
  agent 1:   256 candidates, K = 1, S = 21  a descending list of 65 (some without the flags), detail only
  agent 2:   315 candidates, K = 8          no list, cost with reach-set responsibility
  agent 3: 2 176 candidates, K = 20         a descending list of 241, cost with action-space responsibility and a boundary array
  agent 4:    40 candidates, K = 5          a list of ONE candidate, cost with FX_RISK_BOUNDARY_ARRAY"""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import risk_costs_restatement as rcr
from tests import risk_restatement as rr
from tests.test_predprob_batch_gpu import COUNTS, SHAPES, _engine, _make
from tests.test_resp_batch_gpu import MODES, REACH, _ego, _scene
from tests.test_risk_costs_gpu import COEFF, COLS, WEIGHTS
from tests.test_risk_gpu import HARM

pytestmark = pytest.mark.gpu

NEED = 0xB   # VALID | FEASIBLE | RETURNED
ROWS = ("ego_risk", "obst_risk", "obst_harm_occ")
COSTS = ("bayes", "equality", "maximin", "ego", "responsibility", "total", "boundary_harm")
FIELDS = ROWS + COLS + COSTS + ("min_risk_index", "min_cost_index")   # order of FxRiskCostBatchOutputs


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same(got, want, what=""):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
            assert np.array_equal(_bits(got[k]), _bits(w)), (what, k)
        else:
            assert got[k] == w, (what, k, got[k], w)


def _cp(weights=WEIGHTS, **kw):
    from frenetix_motion_planner_amd import risk
    return risk.risk_cost_params(weights, **kw)


def _forms(scenes):
    """(lists, cost parameters) of the shared call"""
    f1 = scenes[1]["flags"]
    lack, good = np.nonzero((f1 & NEED) != NEED)[0][::3][:20], np.nonzero((f1 & NEED) == NEED)[0]
    l1 = np.sort(np.concatenate([lack, good[:65 - len(lack)]]))[::-1].copy()
    assert len(l1) == 65 and len(lack) > 0 and np.all(np.diff(l1) < 0)
    l3 = np.arange(2170, 5, -9)
    assert len(l3) == 241 and ((scenes[3]["flags"][l3] & NEED) == NEED).sum() > 64
    l4 = np.nonzero((scenes[4]["flags"] & NEED) == NEED)[0][3:4]
    rng = np.random.default_rng(11)
    bh3 = np.where(rng.random(len(l3)) < 0.4, rng.random(len(l3)), 0.0)
    lists = [None, l1, None, l3, l4]
    costs = [None, None, _cp(responsibility="reach_set"), _cp(boundary_harm=bh3, responsibility=scenes[3]["vec"]),
             _cp(boundary_harm=np.array([0.375]), responsibility=scenes[4]["vec"])]
    return lists, costs


def _batch(eng, scenes, lists=None, costs=None, agents=None):
    lst = list(range(len(scenes))) if agents is None else agents
    ids = None if lists is None else [lists[a] for a in lst]
    prm = [scenes[a]["params"] for a in lst]
    if costs is None:
        return eng.risk_detail_batch(prm, ids, agents=agents)
    return eng.risk_costs_batch(prm, [costs[a] for a in lst], ids, agents=agents)


def _solo(eng, scenes, a, ids=None, cost=None):
    if cost is None:
        return eng.risk_detail(scenes[a]["params"], ids, agent=a)
    return eng.risk_costs(scenes[a]["params"], cost, ids, agent=a)


@pytest.fixture(scope="module")
def ctx():
    """one context of five agents with their scenes, the per-agent calls of the mixed forms and the batched call -- computed once,
    left unchanged"""
    inps = [_make(s) for s in SHAPES]
    assert [i.n_candidates for i in inps] == COUNTS and [i.n_samples for i in inps] == [31, 21, 31, 31, 31]
    eng = _engine()
    eng.plan_batch(inps)
    scenes = [_scene(eng, a, s, inps[a], MODES[a], REACH[a]) for a, s in enumerate(SHAPES)]
    lists, costs = _forms(scenes)
    solo = [_solo(eng, scenes, a, lists[a], costs[a]) for a in range(5)]
    batch = _batch(eng, scenes, lists, costs)
    yield eng, inps, scenes, lists, costs, solo, batch
    eng.close()


def test_batch_equals_agents_alone(ctx):
    eng, inps, scenes, lists, costs, solo, batch = ctx
    assert len(batch) == 5 and eng.last_risk_ms > 0
    K = [s["K"] for s in SHAPES]
    n_a = [COUNTS[a] if lists[a] is None else len(lists[a]) for a in range(5)]
    for a in range(5):
        _same(batch[a], solo[a], a)
        assert ("total" in batch[a]) == (costs[a] is not None) == ("min_cost_index" in batch[a])
        assert batch[a]["ego_risk"].shape == (n_a[a],) and batch[a]["ego_risk_max"].shape == (n_a[a], K[a])
    # the per-agent call made after the batch returns the same again
    for a in range(5):
        _same(_solo(eng, scenes, a, lists[a], costs[a]), solo[a], ("per-agent after the batch", a))
    # what the forms mean: NaN rows exactly for the unselected candidates of an agent without a list, listed means evaluated
    for a in (0, 2):
        sel = (scenes[a]["flags"] & NEED) == NEED
        assert sel.any() and (~sel).any()
        for k in ROWS + COLS + (COSTS if costs[a] is not None else ()):
            v = batch[a][k]
            assert np.all(np.isnan(v[~sel])) and not np.isnan(v[sel]).any(), (a, k)
    f1 = scenes[1]["flags"][lists[1]]
    assert ((f1 & NEED) != NEED).any() and not np.isnan(batch[1]["ego_risk"][(f1 & NEED) == NEED]).any()
    assert (batch[2]["ego_risk"][(scenes[2]["flags"] & NEED) == NEED] > 0).any() and (batch[2]["responsibility"] < 0).any()
    assert (batch[3]["ego_risk"] > 0).sum() > 20 and (batch[3]["responsibility"] < 0).any()
    assert (batch[3]["boundary_harm"] > 0).any() and (batch[3]["boundary_harm"] == 0).any()
    assert batch[4]["boundary_harm"].tolist() == [0.375] and batch[4]["min_cost_index"] == lists[4][0] == batch[4]["min_risk_index"]
    assert batch[3]["min_cost_index"] in set(lists[3].tolist()) and batch[1]["min_risk_index"] in set(lists[1].tolist())
    # the views lie in the concatenated arrays: rows at the sums of n_a, columns at the sums of K_a n_a of the agents in front
    off = np.concatenate([[0], np.cumsum(n_a)])
    coff = np.concatenate([[0], np.cumsum([k * n for k, n in zip(K, n_a)])])
    addr = lambda v: v.__array_interface__["data"][0]
    for k in ROWS:
        assert [addr(b[k]) - addr(batch[0][k]) for b in batch] == [8 * int(o) for o in off[:-1]], k
    for k in COLS:
        assert [addr(b[k]) - addr(batch[0][k]) for b in batch] == [8 * int(o) for o in coff[:-1]], k
        assert all(b[k].T.flags["C_CONTIGUOUS"] for b in batch)
    for k in COSTS:
        assert [addr(batch[a][k]) - addr(batch[2][k]) for a in (3, 4)] == [8 * int(off[a] - off[2]) for a in (3, 4)], k


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_tile_edges(ctx, n):
    """the 315-candidate agent listed with n ids beside the others, with cost parameters and a boundary array of that length"""
    eng, inps, scenes, lists, costs, solo, batch = ctx
    l2 = (np.arange(n) * 2 + 5)[::-1].copy()
    assert l2.max() < COUNTS[2]
    ll, cc = list(lists), list(costs)
    ll[2] = l2
    cc[2] = _cp(boundary_harm=np.linspace(0.0, 0.5, n), responsibility="reach_set")
    res = _batch(eng, scenes, ll, cc)
    _same(res[2], _solo(eng, scenes, 2, l2, cc[2]), n)
    for a in (0, 1, 3, 4):
        _same(res[a], solo[a], (n, a))


def test_subsets_and_orders(ctx):
    eng, inps, scenes, lists, costs, solo, batch = ctx
    for agents in ([4, 3, 2, 1, 0], [3, 1], [4], [2, 0, 4]):
        res = _batch(eng, scenes, lists, costs, agents)
        assert len(res) == len(agents)
        for r, a in zip(res, agents):
            _same(r, solo[a], (agents, a))
    # no agent has a list and none has cost parameters: the n_ids == NULL, cost == NULL form
    for r, a in zip(_batch(eng, scenes, None, None, [4, 2]), (4, 2)):
        _same(r, _solo(eng, scenes, a), ("detail, no lists", a))
    # a list with repeated ids: the per-agent call accepts it, so does the batch, with the same rows
    rep = np.array([7, 3, 7, 300, 3, 3, 12])
    cp = _cp(boundary_harm=np.arange(7) / 10.0, responsibility="reach_set")
    want = _solo(eng, scenes, 2, rep, cp)
    assert np.array_equal(_bits(want["ego_risk"][0]), _bits(want["ego_risk"][2])) and want["ego_risk"].shape == (7,)
    got = eng.risk_costs_batch([scenes[2]["params"], scenes[4]["params"]], [cp, costs[4]], [rep, lists[4]], agents=[2, 4])
    _same(got[0], want, "repeated ids"), _same(got[1], solo[4], "beside repeated ids")
    # one parameter object and one cost object for all
    one = _cp(responsibility=None)
    for r, a in zip(eng.risk_costs_batch(scenes[2]["params"], one, [lists[1], None], agents=[1, 2]), (1, 2)):
        _same(r, eng.risk_costs(scenes[2]["params"], one, lists[a], agent=a), ("one params", a))
    # an empty list is a list: no rows, no winner
    e = eng.risk_costs_batch([scenes[1]["params"], scenes[4]["params"]], [_cp(), costs[4]], [np.zeros(0, np.int64), lists[4]], agents=[1, 4])
    assert e[0]["total"].shape == (0,) and e[0]["ego_risk_max"].shape == (0, 1) and e[0]["min_risk_index"] == e[0]["min_cost_index"] == -1
    _same(e[1], solo[4], "beside an empty list")


def test_chunks(ctx):
    """fx_risk_items_set_chunk_steps of 1, 7 and S - 1 against the automatic rule: the same bits"""
    from frenetix_motion_planner_amd._lib import lib
    eng, inps, scenes, lists, costs, solo, batch = ctx
    L = lib()
    try:
        for cs in (1, 7, 30):      # (S - 1 of the four agents with S = 31; agent 1 is capped at its own 20)
            L.fx_risk_items_set_chunk_steps(cs)
            for a, r in enumerate(_batch(eng, scenes, lists, costs)):
                _same(r, solo[a], (cs, a))
    finally:
        L.fx_risk_items_set_chunk_steps(0)
    for a, r in enumerate(_batch(eng, scenes, lists, costs)):
        _same(r, batch[a], a)


def test_rounds(ctx):
    """the 2 176-candidate agent without a list under a scratch limit of four of its tiles: at least three rounds (the call
    reports them), agents sharing rounds, the same bits.  One candidate's share of the scratch: 8 * 7 * K * chunks bytes"""
    from frenetix_motion_planner_amd._lib import lib
    eng, inps, scenes, lists, costs, solo, batch = ctx
    L = lib()
    ll, cc = list(lists), list(costs)
    ll[3] = None
    cc[3] = _cp(responsibility=scenes[3]["vec"])
    want3 = _solo(eng, scenes, 3, None, cc[3])
    share3 = 8 * 7 * 20 * -(-30 // L.fx_risk_items_chunk_steps(COUNTS[3], 31, 20))
    limit = 4 * 64 * share3 + 64 * share3 // 2
    _batch(eng, scenes, ll, cc)
    assert eng.last_risk_costs_batch_rounds == 1
    try:
        for lim, least in ((limit, 3), (1 << 16, 3), (1, 34)):
            L.fx_risk_batch_set_scratch_limit(lim)
            res = _batch(eng, scenes, ll, cc)
            rounds = eng.last_risk_costs_batch_rounds
            print(f"limit {lim} bytes ({share3} per candidate of agent 3): {rounds} rounds")
            assert rounds >= least
            _same(res[3], want3, (lim, 3))
            for a in (0, 1, 2, 4):
                _same(res[a], solo[a], (lim, a))
        L.fx_risk_items_set_chunk_steps(7)
        L.fx_risk_batch_set_scratch_limit(limit)
        res = _batch(eng, scenes, ll, cc)
        assert eng.last_risk_costs_batch_rounds >= 3
        _same(res[3], want3, "both")
    finally:
        L.fx_risk_items_set_chunk_steps(0)
        L.fx_risk_batch_set_scratch_limit(0)
    for a, r in enumerate(_batch(eng, scenes, lists, costs)):
        _same(r, batch[a], a)


def test_ties_go_to_the_candidate_index(ctx):
    """agent 0 (K = 0: every principle 0.0, so every total is equal) listed in descending order returns the SMALLEST listed
    candidate index from both arg-mins, not ids[0]"""
    eng, inps, scenes, lists, costs, solo, batch = ctx
    for l0 in (np.arange(59, 2, -3), np.array([17, 40, 3, 58])):
        ll, cc = list(lists), list(costs)
        ll[0], cc[0] = l0, _cp(responsibility="reach_set")
        res = _batch(eng, scenes, ll, cc)
        assert np.all(res[0]["total"] == 0.0) and np.all(res[0]["ego_risk"] == 0.0)
        assert res[0]["min_cost_index"] == res[0]["min_risk_index"] == l0.min() != l0[0]
        _same(res[0], _solo(eng, scenes, 0, l0, cc[0]))
        _same(res[3], solo[3])


def test_matches_the_restatement(ctx):
    """independent of the code the two calls share: agent 2 (a list, reach-set responsibility, a boundary array) of ONE batched call
    on the device's planes, at the bounds of tests/test_risk_costs_gpu.py; the arg-mins exact"""
    eng, inps, scenes, lists, costs, solo, batch = ctx
    sc = scenes[2]
    K = SHAPES[2]["K"]
    sub = np.nonzero((sc["flags"] & NEED) == NEED)[0][::2]
    rng = np.random.default_rng(5)
    bh = np.where(rng.random(len(sub)) < 0.4, 1.0 / (1.0 + np.exp(-COEFF[0] - COEFF[1] * sc["planes"]["v"][sub, 7])), 0.0)
    ll, cc = list(lists), list(costs)
    ll[2], cc[2] = sub, _cp(boundary_harm=bh, responsibility="reach_set")
    got = _batch(eng, scenes, ll, cc)[2]
    P = [sc["planes"][n][sub] for n in ("x", "y", "theta", "v")]
    want = rcr.calc_risk_detail(*P, sc["preds"], sc["typ"], MODES[2], HARM, **_ego(2))
    we, wo = rr.calc_risk(*P, sc["preds"], sc["typ"], MODES[2], HARM, **_ego(2))
    assert (want["ego_risk"] > 0).sum() > len(sub) // 4, "too few candidates near an obstacle"
    err = lambda g, w: float((np.abs(g - w) / np.maximum(np.abs(w), 1.0)).max())
    for q in COLS + ROWS:
        e = err(got[q], want[q])
        print(f"{q}: {e:.2e} (bound 1e-12)")
        assert e < 1e-12, (q, e)
    assert err(got["ego_risk"], we) < 1e-12 and err(got["obst_risk"], wo) < 1e-12
    wr = [rcr.responsibility_reach_set(P[0][c], P[1][c], inps[2].dt, sc["sets"], want["obst_risk_max"][c], sc["keys"])[0] for c in range(len(sub))]
    wc = rcr.costs(want, bh, WEIGHTS, wr)
    tol = dict(bayes=(2 * K + 1) * 1e-12, equality=(2 * K + 1) * 1e-12, maximin=10e-12, ego=(2 * K + 1) * 1e-12,
               responsibility=(2 * K + 1) * 1e-12)
    tol["total"] = sum(w * tol[n] for w, n in zip(WEIGHTS, rcr.NAMES))
    for q, t in tol.items():
        e = err(got[q], wc[q])
        print(f"{q}: {e:.2e} (bound {t:.1e})")
        assert e < t, (q, e)
    assert np.array_equal(got["boundary_harm"], bh)
    assert got["min_risk_index"] == rr.min_risk_index(got["ego_risk"], got["obst_risk"], sub)
    assert got["min_cost_index"] == rcr.argmin_index(got["total"], sub)


def test_step_boundary_harm():
    """FX_RISK_BOUNDARY_STEP in a batch: an agent whose step ran the road-boundary stage (the scene of
    tests/test_risk_costs_gpu.py) with candidates that carry FX_FLAG_BOUNDARY, beside one whose step did not"""
    from frenetix_motion_planner_amd import _abi, risk
    from tests.test_risk_gpu import BASE, _predictions
    inps = [_make(dict(grid=(4, 8, 12)), n_obstacles=2, road_half_width=1.2), _make(SHAPES[4])]
    assert inps[0].mode & _abi.FX_MODE_ROAD_BOUNDARY and not inps[1].mode & _abi.FX_MODE_ROAD_BOUNDARY
    with _engine(2) as eng:
        eng.plan_batch(inps)
        _, flags = eng.costs(0)
        planes = {n: eng.plane(n, 0).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(3), n_obs=1)
        eng.set_risk_obstacles(risk.obstacle_tables(preds, typ), 0)
        sc1 = _scene(eng, 1, SHAPES[4], inps[1])
        params = [risk.risk_params(dict(BASE, ignore_angle=True), HARM, **_ego(0)), sc1["params"]]
        ids = np.nonzero(flags & _abi.FX_FLAG_SELECTABLE)[0]
        assert (flags[ids] & _abi.FX_FLAG_BOUNDARY).sum() > 5 and (~flags[ids] & _abi.FX_FLAG_BOUNDARY).sum() > 5
        cp = _cp(boundary_harm="step", harm_coeff=COEFF)
        for lists in ([ids, None], [None, None]):
            want = [eng.risk_costs(params[a], cp, lists[a], agent=a) for a in (0, 1)]
            got = eng.risk_costs_batch(params, cp, lists)
            _same(got[0], want[0], "road boundary"), _same(got[1], want[1], "no road boundary")
            assert not got[1]["boundary_harm"][~np.isnan(got[1]["boundary_harm"])].any()
        bh = eng.risk_costs_batch(params, cp, [ids, None])[0]["boundary_harm"]
        on = (flags[ids] & _abi.FX_FLAG_BOUNDARY) != 0
        assert np.all(bh[on] > 0) and np.all(bh[~on] == 0)


def test_sparse_set_agent():
    """a context whose step ran select-only: after materialise(ids) a batch over that agent's ids equals the per-agent call; a
    batch naming an id outside the set is FX_ERR_NOT_READY, outputs untouched"""
    from frenetix_motion_planner_amd import _abi, risk
    inps = [_make(SHAPES[2], write_bundle=False), _make(SHAPES[4])]
    with _engine(2) as eng, _engine(1) as full:
        eng.plan_batch(inps)
        full.plan_batch([_make(SHAPES[2])])
        sc_full = _scene(full, 0, SHAPES[2], inps[0])        # (the planes the obstacles walk along: a bundle-mode twin of agent 0)
        eng.set_risk_obstacles(risk.obstacle_tables(sc_full["preds"], sc_full["typ"]), 0)
        eng.set_reach_sets(risk.reach_set_tables(sc_full["sets"], sc_full["keys"], inps[0].dt, inps[0].n_samples), 0)
        scenes = [dict(sc_full, flags=eng.costs(0)[1]), _scene(eng, 1, SHAPES[4], inps[1])]
        ok = np.nonzero((scenes[0]["flags"] & NEED) == NEED)[0]
        sub = ok[np.arange(len(ok)) % 3 != 1][:70]
        assert len(sub) > 64      # (more than a tile)
        eng.materialise(sub, agent=0)
        order = sub[::-1].copy()
        costs = [_cp(boundary_harm=np.arange(len(order)) / 100.0, responsibility="reach_set"), _cp(responsibility=scenes[1]["vec"])]
        want = [_solo(eng, scenes, 0, order, costs[0]), _solo(eng, scenes, 1, None, costs[1])]
        got = _batch(eng, scenes, [order, None], costs)
        _same(got[0], want[0], "sparse"), _same(got[1], want[1], "beside the sparse one")
        assert got[0]["min_cost_index"] in set(sub.tolist()) and got[0]["min_risk_index"] in set(sub.tolist())
        assert (got[0]["ego_risk"] > 0).any()
        outside = np.setdiff1d(ok, sub)[:1]
        bad = np.concatenate([order[:5], outside])
        r = _raw(eng, [1, 0], scenes, [None, bad], [costs[1], _cp()])
        assert r[0] == _abi.FX_ERR_NOT_READY and "agent 0" in r[1] and "FX_MODE_WRITE_BUNDLE" in r[1] and _untouched(r), r[:2]
        r = _raw(eng, [1, 0], scenes, [None, None])      # (without a list a step without a bundle has nothing to read)
        assert r[0] == _abi.FX_ERR_NOT_READY and "agent 0" in r[1] and _untouched(r), r[:2]
        _same(_batch(eng, scenes, [order, None], costs)[0], want[0], "after the refusals")


def test_nothing_else_moves(ctx):
    eng, inps, scenes, lists, costs, solo, batch = ctx

    def state():
        # (the result block but for the device times it reports, which depend on when it is read)
        block = [{k: repr(v) for k, v in r.items() if "ms" not in k and "time" not in k} for r in eng.finish()]
        sums = [hashlib.sha256(b"".join(eng.plane(n, a).tobytes() for n in ("x", "y", "theta", "v"))).hexdigest() for a in range(5)]
        return [eng.costs(a) for a in range(5)], eng.step_info(), block, sums

    s0 = state()
    bytes0 = eng.device_bytes
    got = _batch(eng, scenes, lists, costs)
    bytes1 = eng.device_bytes
    s1 = state()
    for (c0, f0), (c1, f1) in zip(s0[0], s1[0]):
        assert np.array_equal(c0, c1, equal_nan=True) and np.array_equal(f0, f1)
    assert s0[1] == s1[1] and s0[2] == s1[2] and s0[3] == s1[3] and len(s0[2]) == 5 and "best_index" in s0[2][0]
    for a in range(5):
        _same(got[a], solo[a], a)
    # the only memory is the risk passes' grow-only block: a second call of the same size takes nothing, a larger one grows it
    assert bytes1 >= bytes0
    _batch(eng, scenes, lists, costs)
    assert eng.device_bytes == bytes1
    _batch(eng, scenes, None, None)
    bytes2 = eng.device_bytes
    assert bytes2 >= bytes1
    _batch(eng, scenes, lists, costs)
    assert eng.device_bytes == bytes2
    # NULL output pointers are honoured: total and min_cost_index alone
    r = _raw(eng, [0, 1, 2, 3, 4], scenes, lists, costs, only=("total", "min_cost_index"))
    assert r[0] == 0, r[:2]
    off = np.concatenate([[0], np.cumsum([len(b["ego_risk"]) for b in batch])])
    for a in (2, 3, 4):
        assert np.array_equal(_bits(r[2]["total"][off[a]:off[a + 1]]), _bits(batch[a]["total"])), a
    assert np.all(r[2]["total"][:off[2]] == 7)   # (rows of the agents without cost parameters are left unwritten)
    assert r[2]["min_cost_index"].tolist() == [-1, -1] + [batch[a]["min_cost_index"] for a in (2, 3, 4)]
    assert all(np.all(v == 7) for k, v in r[2].items() if k not in ("total", "min_cost_index"))


def _raw(eng, agents, scenes, lists, costs=None, n=None, only=None, params_null=False, out_null=False, ctx_null=False):
    """the library's call with outputs filled with 7: (status, message, {field: array}); lists[i]: None or ids, or the pair
    (n_ids, None) for a count without a list; costs[i]: None or FxRiskCostParams; only: the fields that get a pointer"""
    from frenetix_motion_planner_amd import _abi
    from frenetix_motion_planner_amd._lib import lib
    n = len(agents) if n is None else n
    m = max(len(agents), 1)
    pi64, pcp = C.POINTER(C.c_int64), C.POINTER(_abi.FxRiskCostParams)
    rows = cols = 0
    keep, cnt, ptr = [], [], []
    for a, x in zip(agents, lists):
        known = 0 <= a < len(eng._inputs)
        if isinstance(x, tuple):
            cnt.append(x[0]), ptr.append(C.cast(None, pi64))
            continue
        if x is None:
            na = eng._inputs[a].n_candidates if known else 0
            cnt.append(0), ptr.append(C.cast(None, pi64))
        else:
            x = np.ascontiguousarray(x, np.int64)
            keep.append(x)
            na = len(x)
            cnt.append(len(x)), ptr.append(x.ctypes.data_as(pi64))
        rows += na
        cols += na * getattr(eng, "_risk_K", {}).get(a, 0)
    arr = {k: np.full(max(cols if k in COLS else rows, 1), 7.0) for k in ROWS + COLS + COSTS}
    arr.update({k: np.full(m, 7, np.int64) for k in ("min_risk_index", "min_cost_index")})
    out = _abi.FxRiskCostBatchOutputs(*[arr[k].ctypes.data if only is None or k in only else None for k in FIELDS])
    sc = [scenes[a if 0 <= a < len(scenes) else 0] for a in agents]
    params = (_abi.FxRiskParams * m)(*[s["params"] for s in sc])
    cpp = None if costs is None else (pcp * m)(*[C.cast(None, pcp) if c is None else C.pointer(c) for c in costs])
    al = np.ascontiguousarray(agents, np.int32)
    n_ids = np.asarray(cnt + [0], np.int64)
    rc = lib().fx_eval_risk_costs_batch(None if ctx_null else eng._ctx, n, al.ctypes.data_as(C.POINTER(C.c_int32)),
                                        None if params_null else params, cpp, n_ids.ctypes.data_as(pi64), (pi64 * m)(*ptr),
                                        None if out_null else C.byref(out))
    return rc, lib().fx_last_error().decode(), arr


def _untouched(r):
    return all(np.all(x == 7) for x in r[2].values())


def test_refusals(ctx):
    from frenetix_motion_planner_amd import _abi
    eng, inps, scenes, lists, costs, solo, batch = ctx
    before = eng.device_bytes
    INV = _abi.FX_ERR_INVALID_ARGUMENT
    five = [0, 1, 2, 3, 4]

    def bad_cost(**kw):
        c = _cp(responsibility=scenes[3]["vec"])
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def with_cost(a, c):
        cc = list(costs)
        cc[a] = c
        return cc

    cases = (("duplicate", _raw(eng, [1, 2, 1], scenes, [lists[1], None, None], [None, costs[2], None]), "agent 1 listed twice"),
             ("out of range", _raw(eng, [0, 5], scenes, [None, None]), "agent 5"),
             ("negative", _raw(eng, [0, -1], scenes, [None, None]), "agent -1"),
             ("too many", _raw(eng, [0, 1, 2, 3, 4, 4], scenes, [None] * 6, n=6), "n_agents 6"),
             ("negative count", _raw(eng, [0], scenes, [None], n=-1), "n_agents -1"),
             ("id out of range", _raw(eng, [3, 2, 4], scenes, [None, np.array([5, COUNTS[2], 7]), None]), "agent 2"),
             ("negative id", _raw(eng, [4, 1], scenes, [np.array([3, -1]), None]), "agent 4"),
             ("a count without a list", _raw(eng, [2, 3], scenes, [None, (4, None)]), "agent 3"),
             ("NULL context", _raw(eng, five, scenes, lists, costs, ctx_null=True), "context"),
             ("NULL out", _raw(eng, five, scenes, lists, costs, out_null=True), "out"),
             ("NULL params", _raw(eng, five, scenes, lists, costs, params_null=True), "params"),
             ("boundary mode", _raw(eng, five, scenes, lists, with_cost(3, bad_cost(boundary_mode=3))), "agent 3: boundary_mode 3"),
             ("array mode without an array", _raw(eng, five, scenes, lists, with_cost(2, bad_cost(boundary_mode=1))), "agent 2: boundary_mode 1"),
             ("responsibility mode", _raw(eng, five, scenes, lists, with_cost(4, bad_cost(responsibility_mode=3))), "agent 4: responsibility_mode 3"),
             ("action space without a vector", _raw(eng, five, scenes, lists, with_cost(3, bad_cost(responsibility=None))),
              "agent 3: responsibility_mode 1"),
             ("ego mass", _raw(eng, [2, 4], [dict(params=_params(2, ego_mass=0.0))] * 5, [None, None]), "agent 2: ego length"))
    for name, r, word in cases:
        assert r[0] == INV and word in r[1] and _untouched(r), (name, r[:2])
    assert str(COUNTS[2]) in cases[5][1][1]
    r = _raw(eng, [0, 1], scenes, [None, None], n=0)
    assert r[0] == _abi.FX_OK and _untouched(r)
    with pytest.raises(ValueError, match="agent 2"):
        eng.risk_costs_batch([scenes[a]["params"] for a in (3, 2)], None, [None, [COUNTS[2]]], agents=[3, 2])
    with pytest.raises(ValueError):
        eng.risk_detail_batch([scenes[0]["params"]], None, agents=[0, 1])
    with pytest.raises(ValueError, match="boundary_harm"):   # (an array that does not cover the agent's rows never reaches the library)
        eng.risk_costs_batch([scenes[4]["params"]], [_cp(boundary_harm=np.zeros(3))], [lists[4]], agents=[4])
    assert eng.device_bytes == before
    # the previous results of a per-agent call are still readable: the refusals touched neither the block nor the tables
    for a in range(5):
        _same(_solo(eng, scenes, a, lists[a], costs[a]), solo[a], ("per-agent after the refusals", a))
    for a, r in enumerate(_batch(eng, scenes, lists, costs)):
        _same(r, solo[a], a)


def test_refusals_of_the_agents_tables():
    """what fx_eval_risk_costs_agent refuses of an agent's obstacle and reach-set tables, in a batch: the same code, the agent
    named, outputs untouched -- an obstacle with min(S - 1, n_pos) == 0, a reach-set entry beyond K, a part beyond the horizon"""
    from frenetix_motion_planner_amd import _abi, risk
    small = [SHAPES[4], SHAPES[0]]
    inps = [_make(s) for s in small]
    with _engine(2) as eng:
        eng.plan_batch(inps)
        scenes = [_scene(eng, a, small[a], inps[a]) for a in range(2)]
        sc = scenes[0]
        cp = _cp(responsibility="reach_set")
        want = eng.risk_costs_batch([s["params"] for s in scenes], cp)
        key = sc["keys"][1]
        empty = dict(sc["preds"][key], pos_list=np.zeros((0, 2)), cov_list=np.zeros((0, 2, 2)), orientation_list=np.zeros(0), v_list=np.zeros(0))
        eng.set_risk_obstacles(risk.obstacle_tables({**sc["preds"], key: empty}, sc["typ"]), 0)
        r = _raw(eng, [1, 0], scenes, [None, None], [cp, cp])
        assert r[0] == _abi.FX_ERR_INVALID_ARGUMENT and "agent 0: obstacle 1" in r[1] and _untouched(r), r[:2]
        with pytest.raises(ValueError):
            eng.risk_detail(sc["params"], agent=0)
        eng.set_risk_obstacles(risk.obstacle_tables(sc["preds"], sc["typ"]), 0)
        good = risk.reach_set_tables(sc["sets"], sc["keys"], inps[0].dt, inps[0].n_samples)
        assert len(good["entry_obs"]) > 0 and len(good["part_step"]) > 0
        for bad, word in ((dict(good, entry_obs=np.full_like(good["entry_obs"], 5)), "reach-set entry 0"),
                          (dict(good, part_step=np.full_like(good["part_step"], inps[0].n_samples)), "reach-set part 0")):
            eng.set_reach_sets(bad, 0)
            r = _raw(eng, [1, 0], scenes, [None, None], [cp, cp])
            assert r[0] == _abi.FX_ERR_INVALID_ARGUMENT and "agent 0" in r[1] and word in r[1] and _untouched(r), r[:2]
            r = _raw(eng, [1, 0], scenes, [None, None], [cp, None])     # (the tables are checked for a cost pass in reach-set mode alone)
            assert r[0] == _abi.FX_OK, r[:2]
        eng.set_reach_sets(good, 0)
        for g, w in zip(eng.risk_costs_batch([s["params"] for s in scenes], cp), want):
            _same(g, w, "after the refusals")


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
        costs = [_cp(), _cp(responsibility=scenes[1]["vec"])]
        want = _batch(eng, scenes, lists, costs)
        eng.update_state(eng.make_state_update(v_des=inps[1].v_des + 1.0), agent=1)
        r = _raw(eng, [1, 0], scenes, [None, lists[0]], [costs[1], costs[0]])
        assert r[0] == _abi.FX_ERR_NOT_READY and "rewritten" in r[1] and "agent 1" in r[1] and _untouched(r), r[:2]
        eng.evaluate()
        eng.finish()
        again = _batch(eng, scenes, lists, costs)
        _same(again[0], want[0], "agent 0's inputs are what they were")
        _same(again[1], _solo(eng, scenes, 1, None, costs[1]), "agent 1 after its new step")


def _params(a, **kw):
    """agent a's parameters; kw: fields overwritten afterwards (values the Python layer would refuse itself)"""
    from frenetix_motion_planner_amd import risk
    p = risk.risk_params(MODES[0], HARM, **_ego(a))
    for k, v in kw.items():
        setattr(p, k, v)
    return p
