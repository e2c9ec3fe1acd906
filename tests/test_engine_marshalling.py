"""What FrenetEngine's pass wrappers hand to the library, per-agent and batched, without a GPU: the engine is made with __new__,
its inputs are stand-ins, and `engine.lib` is replaced by a recorder that decodes every argument DURING the call (the pointers die
afterwards) into plain Python -- ints, None for NULL, lists copied out of the pointed-to arrays with the lengths the ABI implies,
structure fields by name -- writes recognisable values into the outputs and returns 0.  The recorder holds every argument to the
real entry point's argtypes, so what ctypes would refuse is refused here as well.  The expectations are written out below.

The upload: three agents with 5, 0 and 7 candidates and (K, P) of (2, 3), (0, 0) and (1, 2) -- the smallest shapes that tell
offsets, an empty agent and differing strides apart."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, _lib
from frenetix_motion_planner_amd import engine as E
from frenetix_motion_planner_amd.engine import FrenetEngine

N_CAND = [5, 0, 7]
KP = [(2, 3), (0, 0), (1, 2)]
RISK_K = {0: 2, 2: 1}      # (agent 1 never had risk obstacles: 0)
S = 4
COSTS = [["acceleration", "prediction", "velocity_offset"], [], ["jerk", "prediction"]]
STORED = [(True, True, {"n": 1}), (True, True, None), (False, False, None)]     # write_bundle, write_costmap, _bound
ROW_NAMES = ["ego_risk", "obst_risk", "obst_harm_occ"]
COL_NAMES = ["ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max"]
COST_NAMES = ["bayes", "equality", "maximin", "ego", "responsibility", "total", "boundary_harm"]
INDEX_NAMES = ["min_risk_index", "min_cost_index"]
PARTS = ("planes", "co", "tl", "raw", "cost", "flags", "bst")


def _addr(x):
    """the address an argument or a structure field stands for, None for NULL"""
    if x is None:
        return None
    if isinstance(x, int):
        return x or None
    if isinstance(x, C.c_void_p):
        return x.value
    if isinstance(x, C._Pointer):
        return C.cast(x, C.c_void_p).value
    if isinstance(x, (C.Array, C.Structure)):
        return C.addressof(x)
    return C.addressof(x._obj)      # (byref)


def _read(x, typ, n):
    a = _addr(x)
    return None if a is None else list((typ * int(n)).from_address(a))


def _write(x, typ, values):
    a, values = _addr(x), list(values)
    if a is not None and values:
        (typ * len(values)).from_address(a)[:] = values


def _bound(o):
    return [n for n, _ in o._fields_ if getattr(o, n)]


class Recorder:
    def __init__(self, inputs, risk_K):
        self.inputs, self.risk_K, self.calls = inputs, risk_K, []
        self.real = _lib.lib()

    def __getattr__(self, name):
        if not name.startswith("fx_"):
            raise AttributeError(name)
        decode = getattr(type(self), "_" + name)      # (an entry point nobody expected: AttributeError)
        types = getattr(self.real, name).argtypes

        def call(*args):
            assert len(args) == len(types), name
            for t, a in zip(types, args):
                t.from_param(a)
            self.calls.append((name, decode(self, *args[1:])))
            return 0
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls

    def n_of(self, a):
        return self.inputs[a].n_candidates if 0 <= a < len(self.inputs) else 0

    # -- the risk family --
    def risk_lists(self, n, al, n_ids, idp):
        agents = _read(al, C.c_int32, n)
        nid = _read(n_ids, C.c_int64, n + 1)      # (with the trailing 0 the wrappers append)
        lists = None if _addr(idp) is None else [_read(idp[i], C.c_int64, nid[i]) for i in range(n)]
        listed = agents if agents is not None else list(range(n))
        rows = [self.n_of(a) if lists is None or lists[i] is None else len(lists[i]) for i, a in enumerate(listed)]
        return agents, nid, lists, listed, rows

    def _fx_eval_risk_agent(self, agent, params, n_ids, idp, ego, obst, idx):
        rows = n_ids if _addr(idp) is not None else self.n_of(agent)
        _write(ego, C.c_double, np.arange(rows) + 0.5)
        _write(obst, C.c_double, np.arange(rows) + 100.5)
        idx._obj.value = 3
        return dict(agent=agent, params=params._obj.ego_length, n_ids=n_ids, ids=_read(idp, C.c_int64, n_ids))

    def _fx_eval_risk_batch(self, n, al, prm, n_ids, idp, out):
        agents, nid, lists, listed, rows = self.risk_lists(n, al, n_ids, idp)
        o = out._obj
        _write(o.ego_risk, C.c_double, np.arange(sum(rows)) + 0.5)
        _write(o.obst_risk, C.c_double, np.arange(sum(rows)) + 100.5)
        _write(o.min_risk_index, C.c_int64, [7 + i for i in range(n)])
        return dict(n=n, agents=agents, params=[prm[i].ego_length for i in range(n)], n_ids=nid, ids=lists)

    def _fx_eval_risk_costs_agent(self, agent, params, cp, n_ids, idp, out):
        rows = n_ids if _addr(idp) is not None else self.n_of(agent)
        K, o = self.risk_K.get(agent, 0), out._obj
        for k in _bound(o):
            if k in COL_NAMES:
                _write(getattr(o, k), C.c_double, np.arange(K * max(rows, 1)) + 0.25)      # [K][max(n, 1)]
            elif k not in INDEX_NAMES:
                _write(getattr(o, k), C.c_double, np.arange(rows) + 0.5)
        _write(o.min_risk_index, C.c_int64, [3])
        _write(o.min_cost_index, C.c_int64, [4])
        return dict(agent=agent, params=params._obj.ego_length, cost=None if cp is None else cp._obj.maximin_eps, n_ids=n_ids,
                    ids=_read(idp, C.c_int64, n_ids), bound=_bound(o))

    def _fx_eval_risk_costs_batch(self, n, al, prm, cpp, n_ids, idp, out):
        agents, nid, lists, listed, rows = self.risk_lists(n, al, n_ids, idp)
        cols = sum(self.risk_K.get(a, 0) * m for a, m in zip(listed, rows))
        o = out._obj
        for k in _bound(o):
            if k in COL_NAMES:
                _write(getattr(o, k), C.c_double, np.arange(cols) + 0.25)
            elif k not in INDEX_NAMES:
                _write(getattr(o, k), C.c_double, np.arange(sum(rows)) + 0.5)
        _write(o.min_risk_index, C.c_int64, [7 + i for i in range(n)])
        _write(o.min_cost_index, C.c_int64, [70 + i for i in range(n)])
        cost = None if _addr(cpp) is None else [cpp[i].contents.maximin_eps if cpp[i] else None for i in range(n)]
        return dict(n=n, agents=agents, params=[prm[i].ego_length for i in range(n)], cost=cost, n_ids=nid, ids=lists, bound=_bound(o))

    def _fx_eval_prediction_prob_agent(self, agent, params, n_ids, idp, out):
        rows = n_ids if _addr(idp) is not None else self.n_of(agent)
        K, o, p = self.risk_K.get(agent, 0), out._obj, params._obj
        _write(o.prob, C.c_double, np.arange(rows) + 0.5)
        _write(o.total, C.c_double, np.arange(rows) + 100.5)
        _write(o.prob_obs, C.c_double, np.arange(K * max(rows, 1)) + 0.25)
        _write(o.best_index, C.c_int64, [3])
        _write(o.best_cost, C.c_double, [3.5])
        return dict(agent=agent, params=(p.ego_length, p.ego_width, p.source), n_ids=n_ids, ids=_read(idp, C.c_int64, n_ids),
                    bound=_bound(o))

    def _fx_eval_prediction_prob_batch(self, n, al, params, out):
        agents = _read(al, C.c_int32, n)
        total = sum(self.n_of(a) for a in (agents if agents is not None else range(n)))
        o = out._obj
        _write(o.prob, C.c_double, np.arange(total) + 0.5)
        _write(o.total, C.c_double, np.arange(total) + 100.5)
        _write(o.best_index, C.c_int64, [7 + i for i in range(n)])
        _write(o.best_cost, C.c_double, [7.5 + i for i in range(n)])
        return dict(n=n, agents=agents, params=[(params[i].ego_length, params[i].ego_width, params[i].source) for i in range(n)])

    def resp_params(self, r, rows):
        return dict(weight=r.weight, mode=r.responsibility_mode, responsibility=r.responsibility,
                    prediction=_read(r.prediction, C.c_double, rows))

    def _fx_eval_responsibility_cost_agent(self, agent, params, rp, n_ids, idp, out):
        rows = n_ids if _addr(idp) is not None else self.n_of(agent)
        o = out._obj
        for j, k in enumerate(("resp", "total", "ego_risk", "obst_risk")):
            _write(getattr(o, k), C.c_double, np.arange(rows) + 100 * j + 0.5)
        _write(o.best_index, C.c_int64, [3])
        _write(o.best_cost, C.c_double, [3.5])
        return dict(agent=agent, params=params._obj.ego_length, rp=self.resp_params(rp._obj, rows), n_ids=n_ids,
                    ids=_read(idp, C.c_int64, n_ids))

    def _fx_eval_responsibility_cost_batch(self, n, al, prm, rps, out):
        agents = _read(al, C.c_int32, n)
        listed = agents if agents is not None else list(range(n))
        total = sum(self.n_of(a) for a in listed)
        o = out._obj
        for j, k in enumerate(("resp", "total", "ego_risk", "obst_risk")):
            _write(getattr(o, k), C.c_double, np.arange(total) + 100 * j + 0.5)
        _write(o.best_index, C.c_int64, [7 + i for i in range(n)])
        _write(o.best_cost, C.c_double, [7.5 + i for i in range(n)])
        return dict(n=n, agents=agents, params=[prm[i].ego_length for i in range(n)],
                    rp=[self.resp_params(rps[i], self.n_of(a)) for i, a in enumerate(listed)])

    # -- hypotheses --
    def hyp_entry(self, y, agent):
        K, P = (self.inputs[agent].obstacles[k] for k in "KP") if 0 <= agent < len(self.inputs) else (0, 0)
        return dict(pos=_read(y.obs_pos, C.c_double, 2 * K * P), cov_inv=_read(y.obs_cov_inv, C.c_double, 4 * K * P),
                    npred=_read(y.obs_npred, C.c_int32, K), hull=_read(y.obs_hull, C.c_double, 6 * K * max(P - 1, 0)),
                    nhull=_read(y.obs_nhull, C.c_int32, K))

    def hyp_write(self, o, pairs, cells):
        _write(o.winner, C.c_int64, np.arange(pairs))
        _write(o.cost, C.c_double, np.arange(pairs) + 0.5)
        _write(o.n_collisions, C.c_int64, np.arange(pairs) + 10)
        _write(o.pred, C.c_double, np.arange(cells) + 0.25)
        _write(o.total, C.c_double, np.arange(cells) + 0.75)
        _write(o.collision, C.c_uint8, np.arange(cells) % 2)

    def _fx_eval_hypotheses_agent(self, agent, n_hyp, hyp, out):
        self.hyp_write(out._obj, n_hyp, n_hyp * self.n_of(agent))
        return dict(agent=agent, n_hyp=n_hyp, hyp=[self.hyp_entry(hyp[h], agent) for h in range(n_hyp)], bound=_bound(out._obj))

    def _fx_eval_hypotheses_batch(self, n, ids, n_hyp, hyp, out):
        agents, nh = _read(ids, C.c_int32, n), _read(n_hyp, C.c_int32, n)
        self.hyp_write(out._obj, sum(nh), sum(h * self.n_of(a) for a, h in zip(agents, nh)))
        owner = [a for a, h in zip(agents, nh) for _ in range(h)]
        return dict(n=n, agents=agents, n_hyp=nh, hyp=[self.hyp_entry(hyp[j], a) for j, a in enumerate(owner)], bound=_bound(out._obj))

    def _fx_last_hypotheses_info(self, a, b, c):
        a._obj.value, b._obj.value, c._obj.value = 1, 2, 3

    _fx_last_materialise_info = _fx_last_hypotheses_info

    # -- re-score --
    def n_cost(self, a):
        return len(self.inputs[a].cost_names) if 0 <= a < len(self.inputs) else 0

    def _fx_rescore_agent(self, agent, n_vec, w, winner, cost, tot):
        _write(winner, C.c_int64, np.arange(n_vec) + 100 * agent)
        _write(cost, C.c_double, np.arange(n_vec) + 0.5)
        _write(tot, C.c_double, np.arange(n_vec * self.n_of(agent)) + 0.25)
        return dict(agent=agent, n_vec=n_vec, w=_read(w, C.c_double, n_vec * self.n_cost(agent)), totals=_addr(tot) is not None)

    def _fx_rescore_agent_rows(self, agent, n_vec, w, pred, resp, winner, cost, tot):
        d = self._fx_rescore_agent(agent, n_vec, None, winner, cost, tot)
        width = self.n_cost(agent) + (_addr(resp) is not None)
        return dict(d, w=_read(w, C.c_double, n_vec * width), pred=_read(pred, C.c_double, self.n_of(agent)),
                    resp=_read(resp, C.c_double, self.n_of(agent)))

    def _fx_rescore_batch(self, n, ids, n_vec, w, pred, resp, winner, cost):
        agents, nv = _read(ids, C.c_int32, n), _read(n_vec, C.c_int32, n)
        table = lambda t: None if _addr(t) is None else [_read(p, C.c_double, self.n_of(a)) for p, a in zip(_read(t, C.c_void_p, n), agents)]
        pred, resp = table(pred), table(resp)
        width = [self.n_cost(a) + (resp is not None and resp[i] is not None) for i, a in enumerate(agents)]
        flat = _read(w, C.c_double, sum(k * m for k, m in zip(nv, width)))
        _write(winner, C.c_int64, np.arange(sum(nv)))
        _write(cost, C.c_double, np.arange(sum(nv)) + 0.5)
        return dict(n=n, agents=agents, n_vec=nv, w=flat, pred=pred, resp=resp)

    # -- candidate rows --
    def _fx_read_candidates_agent(self, agent, n, ids, planes, co, tl, raw, cost, flags, bst):
        inp, idl = self.inputs[agent], _read(ids, C.c_int64, n)
        nc = len(inp.cost_names)
        _write(planes, C.c_double, [float(i) for i in idl for _ in range(_abi.FX_NUM_PLANES * inp.n_samples)])
        _write(co, C.c_double, [i + c / 100 for i in idl for c in range(13)])
        _write(tl, C.c_int32, idl)
        _write(raw, C.c_double, [10.0 * i + c for i in idl for c in range(nc)])
        _write(cost, C.c_double, [float(i) for i in idl])       # (each row's id: the permutation back shows in the result)
        _write(flags, C.c_uint32, idl)
        _write(bst, C.c_int32, idl)
        given = (planes, co, tl, raw, cost, flags, bst)
        return dict(agent=agent, n=n, ids=idl, null=[k for k, p in zip(PARTS, given) if _addr(p) is None])

    _fx_read_materialised_agent = _fx_read_candidates_agent

    def _fx_materialise_candidates_agent(self, agent, n, ids):
        return dict(agent=agent, n=n, ids=_read(ids, C.c_int64, n))

    def _fx_materialise_candidates_batch(self, n, ag, n_ids, addr):
        nid, table = _read(n_ids, C.c_int64, n), _read(addr, C.c_uint64, n)
        return dict(n=n, agents=_read(ag, C.c_int32, n), n_ids=nid,
                    ids=None if table is None else [_read(int(a), C.c_int64, k) for a, k in zip(table, nid)])

    def _fx_read_ranked_agent(self, agent, first, n, ids, cost, flags):
        return dict(agent=agent, first=first, n=n, null=[k for k, p in zip(("ids", "cost", "flags"), (ids, cost, flags)) if _addr(p) is None])


@pytest.fixture
def eng(monkeypatch):
    e = FrenetEngine.__new__(FrenetEngine)
    e._ctx = C.c_void_p()
    e._inputs = [SimpleNamespace(n_candidates=n, n_samples=S, cost_names=list(names), obstacles=dict(K=k, P=p), write_bundle=b,
                                 write_costmap=m, _bound=bound)
                 for n, (k, p), names, (b, m, bound) in zip(N_CAND, KP, COSTS, STORED)]
    e._risk_K = dict(RISK_K)
    e.sort_serials = {}
    e._steps = []      # (__del__ stays quiet)
    rec = Recorder(e._inputs, e._risk_K)
    monkeypatch.setattr(E, "lib", lambda: rec)
    return e, rec


def prm(ego_length=4.5, ego_width=1.8):
    return _abi.FxRiskParams(ego_length=ego_length, ego_width=ego_width)


def cost_prm(eps=0.5, mode=_abi.FX_RISK_RESP_ACTION_SPACE, **lengths):
    cp = _abi.FxRiskCostParams(maximin_eps=eps, responsibility_mode=mode)
    cp._keep = np.arange(3.0)
    cp.responsibility = cp._keep.ctypes.data
    if lengths:
        cp._lengths = lengths
    return cp


def same(a, b):
    return a.dtype == np.asarray(b).dtype and a.shape == np.asarray(b).shape and np.array_equal(a, b)


def one_base(views):
    """every view is a slice of ONE array that owns its memory"""
    roots = []
    for v in views:
        while v.base is not None:
            v = v.base
        roots.append(v)
    return all(r is roots[0] for r in roots)


# ---- risk_batch / risk_detail_batch / risk_costs_batch ----
def test_risk_batch(eng):
    e, rec = eng
    out = e.risk_batch(prm(4.5))
    assert rec.take() == [("fx_eval_risk_batch", dict(n=3, agents=None, params=[4.5, 4.5, 4.5], n_ids=None, ids=None))]
    assert [len(r[0]) for r in out] == [5, 0, 7] and [r[2] for r in out] == [7, 8, 9]
    assert same(out[0][0], np.arange(0, 5) + 0.5) and same(out[2][0], np.arange(5, 12) + 0.5) and same(out[2][1], np.arange(5, 12) + 100.5)
    assert one_base([r[0] for r in out]) and one_base([r[1] for r in out])

    out = e.risk_batch([prm(1.0), prm(2.0)], agents=[2, 0])
    assert rec.take() == [("fx_eval_risk_batch", dict(n=2, agents=[2, 0], params=[1.0, 2.0], n_ids=None, ids=None))]
    assert same(out[0][0], np.arange(0, 7) + 0.5) and same(out[1][0], np.arange(7, 12) + 0.5)

    out = e.risk_batch(prm(4.5), ids=[None, [], [3, 1]])
    assert rec.take() == [("fx_eval_risk_batch", dict(n=3, agents=None, params=[4.5] * 3, n_ids=[0, 0, 2, 0], ids=[None, [], [3, 1]]))]
    assert [len(r[0]) for r in out] == [5, 0, 2]
    assert same(out[2][1], np.arange(5, 7) + 100.5) and one_base([r[0] for r in out])

    out = e.risk_batch(prm(4.5), agents=[0, 9])      # (an agent the library will refuse counts no rows)
    assert [len(r[0]) for r in out] == [5, 0] and rec.take()[0][1]["agents"] == [0, 9]
    with pytest.raises(ValueError, match="^1 params and 3 id lists for 3 agents$"):
        e.risk_batch([prm()])
    with pytest.raises(ValueError, match="^3 params and 2 id lists for 3 agents$"):
        e.risk_batch(prm(), ids=[None, None])
    assert rec.take() == []


def test_risk_per_agent(eng):
    e, rec = eng
    ego, obst, idx = e.risk(prm(4.5), agent=2)
    assert rec.take() == [("fx_eval_risk_agent", dict(agent=2, params=4.5, n_ids=0, ids=None))]
    assert same(ego, np.arange(7) + 0.5) and same(obst, np.arange(7) + 100.5) and idx == 3
    ego, obst, idx = e.risk(prm(4.5), ids=[3, 1])
    assert rec.take() == [("fx_eval_risk_agent", dict(agent=0, params=4.5, n_ids=2, ids=[3, 1]))] and len(ego) == 2


def detail_keys(cost):
    return ROW_NAMES + (COST_NAMES if cost else []) + COL_NAMES + ["min_risk_index"] + (["min_cost_index"] if cost else [])


def test_risk_detail_and_costs_batch(eng):
    e, rec = eng
    out = e.risk_detail_batch(prm(4.5), ids=[None, [], [3, 1]])
    assert rec.take() == [("fx_eval_risk_costs_batch", dict(n=3, agents=None, params=[4.5] * 3, cost=None, n_ids=[0, 0, 2, 0],
                                                            ids=[None, [], [3, 1]], bound=ROW_NAMES + COL_NAMES + INDEX_NAMES))]
    assert all(list(d) == detail_keys(False) for d in out)
    assert [len(d["ego_risk"]) for d in out] == [5, 0, 2] and [d["min_risk_index"] for d in out] == [7, 8, 9]
    assert same(out[0]["obst_harm_occ"], np.arange(0, 5) + 0.5) and same(out[2]["obst_harm_occ"], np.arange(5, 7) + 0.5)
    assert [d["ego_harm_max"].shape for d in out] == [(5, 2), (0, 0), (2, 1)]
    assert same(out[0]["ego_harm_max"], (np.arange(0, 10) + 0.25).reshape(2, 5).T)        # [n, K] views of obstacle-major blocks
    assert same(out[2]["ego_harm_max"], (np.arange(10, 12) + 0.25).reshape(1, 2).T)
    for k in ROW_NAMES + COL_NAMES:
        assert one_base([d[k] for d in out]), k

    out = e.risk_detail_batch(prm(4.5))
    assert rec.take() == [("fx_eval_risk_costs_batch", dict(n=3, agents=None, params=[4.5] * 3, cost=None, n_ids=None, ids=None,
                                                            bound=ROW_NAMES + COL_NAMES + INDEX_NAMES))]
    assert [d["obst_risk_max"].shape for d in out] == [(5, 2), (0, 0), (7, 1)]

    # cost_params: one structure for all, a list with a None member, None
    every = ROW_NAMES + COL_NAMES + COST_NAMES + INDEX_NAMES
    out = e.risk_costs_batch([prm(1.0), prm(2.0)], cost_prm(0.5), agents=[2, 0])
    assert rec.take() == [("fx_eval_risk_costs_batch", dict(n=2, agents=[2, 0], params=[1.0, 2.0], cost=[0.5, 0.5], n_ids=None, ids=None,
                                                            bound=every))]
    assert all(list(d) == detail_keys(True) for d in out) and [d["min_cost_index"] for d in out] == [70, 71]
    assert same(out[1]["total"], np.arange(7, 12) + 0.5) and one_base([d["total"] for d in out])
    assert [d["ego_risk_max"].shape for d in out] == [(7, 1), (5, 2)]
    assert same(out[1]["ego_risk_max"], (np.arange(7, 17) + 0.25).reshape(2, 5).T)

    out = e.risk_costs_batch(prm(4.5), [cost_prm(0.25), None, cost_prm(0.75)], ids=[None, [], [3, 1]])
    assert rec.take() == [("fx_eval_risk_costs_batch", dict(n=3, agents=None, params=[4.5] * 3, cost=[0.25, None, 0.75],
                                                            n_ids=[0, 0, 2, 0], ids=[None, [], [3, 1]], bound=every))]
    assert [list(d) for d in out] == [detail_keys(True), detail_keys(False), detail_keys(True)]

    out = e.risk_costs_batch(prm(4.5), None)
    assert rec.take()[0][1]["cost"] is None and all(list(d) == detail_keys(False) for d in out)

    with pytest.raises(ValueError, match="^3 params, 2 cost params and 3 id lists for 3 agents$"):
        e.risk_costs_batch(prm(), [None, None])
    # the arrays behind the structures' pointers must cover what the library reads
    with pytest.raises(ValueError, match="^agent 0: boundary_harm has 4 entries for 5 candidates$"):
        e.risk_costs_batch(prm(), cost_prm(boundary_harm=4, responsibility=7))
    with pytest.raises(ValueError, match="^agent 2: responsibility has 3 entries for 1 obstacles$"):
        e.risk_costs_batch(prm(), cost_prm(responsibility=3), agents=[2])
    e.risk_costs_batch(prm(), cost_prm(boundary_harm=2, responsibility=1), ids=[[3, 1]], agents=[2])      # (what covers passes)
    assert len(rec.take()) == 1


def test_risk_detail_and_costs_per_agent(eng):
    e, rec = eng
    d = e.risk_detail(prm(4.5), ids=[3, 1], agent=2)
    assert rec.take() == [("fx_eval_risk_costs_agent", dict(agent=2, params=4.5, cost=None, n_ids=2, ids=[3, 1],
                                                            bound=ROW_NAMES + COL_NAMES + INDEX_NAMES))]
    assert list(d) == detail_keys(False) and d["min_risk_index"] == 3
    assert same(d["ego_risk"], np.arange(2) + 0.5) and same(d["obst_harm_max"], (np.arange(2) + 0.25).reshape(1, 2).T)
    d = e.risk_costs(prm(4.5), cost_prm(0.5))
    assert rec.take() == [("fx_eval_risk_costs_agent", dict(agent=0, params=4.5, cost=0.5, n_ids=0, ids=None,
                                                            bound=ROW_NAMES + COL_NAMES + COST_NAMES + INDEX_NAMES))]
    assert list(d) == detail_keys(True) and (d["min_risk_index"], d["min_cost_index"]) == (3, 4)
    assert d["ego_risk_max"].shape == (5, 2) and same(d["ego_risk_max"], (np.arange(10) + 0.25).reshape(2, 5).T)
    assert same(d["boundary_harm"], np.arange(5) + 0.5)
    # an empty id list, and an agent without candidates: nothing to evaluate, no call, no arg-min
    d = e.risk_costs(prm(), cost_prm(), ids=[])
    assert rec.take() == [] and d["min_risk_index"] == -1 and d["min_cost_index"] == -1 and d["ego_risk_max"].shape == (0, 2)
    assert e.risk_detail(prm(), agent=1)["ego_risk"].shape == (0,) and rec.take() == []
    with pytest.raises(ValueError, match="^boundary_harm has 4 entries for 5 candidates$"):
        e.risk_costs(prm(), cost_prm(boundary_harm=4, responsibility=7))
    with pytest.raises(ValueError, match="^responsibility has 3 entries for 1 obstacles$"):
        e.risk_costs(prm(), cost_prm(responsibility=3), agent=2)
    assert rec.take() == []


# ---- prediction_probability* and responsibility_cost* ----
def test_prediction_probability(eng):
    e, rec = eng
    out = e.prediction_probability_batch(4.5, 1.8)
    assert rec.take() == [("fx_eval_prediction_prob_batch", dict(n=3, agents=None, params=[(4.5, 1.8, 0)] * 3))]
    assert list(out[0]) == ["prob", "total", "best_index", "best_cost"]
    assert [len(d["prob"]) for d in out] == [5, 0, 7] and same(out[2]["prob"], np.arange(5, 12) + 0.5)
    assert same(out[2]["total"], np.arange(5, 12) + 100.5) and one_base([d["prob"] for d in out]) and one_base([d["total"] for d in out])
    assert [(d["best_index"], d["best_cost"]) for d in out] == [(7, 7.5), (8, 8.5), (9, 9.5)]
    out = e.prediction_probability_batch([4.0, 5.0, 6.0], 1.8, agents=[2, 5, 0], source="step")      # (5: out of range, no rows)
    assert rec.take() == [("fx_eval_prediction_prob_batch", dict(n=3, agents=[2, 5, 0], params=[(4.0, 1.8, 1), (5.0, 1.8, 1), (6.0, 1.8, 1)]))]
    assert [len(d["prob"]) for d in out] == [7, 0, 5] and same(out[2]["prob"], np.arange(7, 12) + 0.5)
    for call in (lambda: e.prediction_probability_batch(4.5, 1.8, source="x"), lambda: e.prediction_probability(4.5, 1.8, source="x")):
        with pytest.raises(ValueError, match=r"^source 'x': one of \['probability', 'step'\]$"):
            call()

    d = e.prediction_probability(4.5, 1.8, agent=2, per_obstacle=True)
    assert rec.take() == [("fx_eval_prediction_prob_agent", dict(agent=2, params=(4.5, 1.8, 0), n_ids=0, ids=None,
                                                                 bound=["prob", "prob_obs", "total", "best_index", "best_cost"]))]
    assert list(d) == ["prob", "total", "prob_obs", "best_index", "best_cost"] and d["prob_obs"].shape == (7, 1)
    assert same(d["prob"], np.arange(7) + 0.5) and (d["best_index"], d["best_cost"]) == (3, 3.5)
    d = e.prediction_probability(4.5, 1.8, ids=[3, 1])
    assert rec.take() == [("fx_eval_prediction_prob_agent", dict(agent=0, params=(4.5, 1.8, 0), n_ids=2, ids=[3, 1],
                                                                 bound=["prob", "total", "best_index", "best_cost"]))]
    assert e.prediction_probability(4.5, 1.8, ids=[])["best_index"] == -1 and rec.take() == []      # (an empty list: no call)
    assert len(e.prediction_probability(4.5, 1.8, agent=1)["prob"]) == 0 and len(rec.take()) == 1   # (every candidate of none: a call)


def test_responsibility_cost_batch(eng):
    e, rec = eng
    params, cps = [prm(4.0, 1.7), prm(5.0, 1.8), prm(6.0, 1.9)], [cost_prm(), cost_prm(mode=_abi.FX_RISK_RESP_REACH_SET), cost_prm()]
    out = e.responsibility_cost_batch(params, cps, [1, 2.5, -3.0], prediction=["step", "probability", "step"])
    calls = rec.take()
    # exactly one probability call, over agent 1, before the responsibility call
    assert [c[0] for c in calls] == ["fx_eval_prediction_prob_batch", "fx_eval_responsibility_cost_batch"]
    assert calls[0][1] == dict(n=1, agents=[1], params=[(5.0, 1.8, 0)])
    mode = [_abi.FX_RISK_RESP_ACTION_SPACE, _abi.FX_RISK_RESP_REACH_SET, _abi.FX_RISK_RESP_ACTION_SPACE]
    assert calls[1][1] == dict(n=3, agents=None, params=[4.0, 5.0, 6.0], rp=[
        dict(weight=w, mode=m, responsibility=cp.responsibility, prediction=None) for w, m, cp in zip([1.0, 2.5, -3.0], mode, cps)])
    assert [list(d) for d in out] == [["resp", "total", "ego_risk", "obst_risk", "best_index", "best_cost", "prediction"]] * 3
    assert [len(d["resp"]) for d in out] == [5, 0, 7] and same(out[2]["ego_risk"], np.arange(5, 12) + 200.5)
    assert [(d["best_index"], d["best_cost"]) for d in out] == [(7, 7.5), (8, 8.5), (9, 9.5)]
    assert out[0]["prediction"] is None and len(out[1]["prediction"]) == 0 and out[2]["prediction"] is None
    for k in ("resp", "total", "ego_risk", "obst_risk"):
        assert one_base([d[k] for d in out]), k

    out = e.responsibility_cost_batch(params[:2], cps[:2], [1.0, 2.0], agents=[2, 0], prediction="probability")
    calls = rec.take()
    assert calls[0] == ("fx_eval_prediction_prob_batch", dict(n=2, agents=[2, 0], params=[(4.0, 1.7, 0), (5.0, 1.8, 0)]))
    assert calls[1][1]["agents"] == [2, 0] and len(calls) == 2
    assert calls[1][1]["rp"][0]["prediction"] == list(np.arange(0, 7) + 0.5) and calls[1][1]["rp"][1]["prediction"] == list(np.arange(7, 12) + 0.5)
    assert same(out[1]["prediction"], np.arange(7, 12) + 0.5) and [len(d["total"]) for d in out] == [7, 5]

    out = e.responsibility_cost_batch(params, cps, [1.0] * 3, agents=[2, 7, 0])      # (7: out of range, no rows)
    assert [len(d["resp"]) for d in out] == [7, 0, 5] and same(out[2]["resp"], np.arange(7, 12) + 0.5) and len(rec.take()) == 1


def test_responsibility_cost(eng):
    e, rec = eng
    cp = cost_prm()
    d = e.responsibility_cost(prm(4.5), cp, 2, ids=[3, 1], agent=2)
    assert rec.take() == [("fx_eval_responsibility_cost_agent", dict(agent=2, params=4.5, n_ids=2, ids=[3, 1], rp=dict(
        weight=2.0, mode=_abi.FX_RISK_RESP_ACTION_SPACE, responsibility=cp.responsibility, prediction=None)))]
    assert list(d) == ["resp", "total", "ego_risk", "obst_risk", "best_index", "best_cost", "prediction"]
    assert same(d["total"], np.arange(2) + 100.5) and (d["best_index"], d["best_cost"], d["prediction"]) == (3, 3.5, None)
    d = e.responsibility_cost(prm(4.5, 1.8), cp, 2.0, ids=[3, 1], prediction="probability")
    calls = rec.take()
    assert [c[0] for c in calls] == ["fx_eval_prediction_prob_agent", "fx_eval_responsibility_cost_agent"]
    assert calls[0][1]["params"] == (4.5, 1.8, 0) and calls[0][1]["ids"] == [3, 1] and calls[1][1]["rp"]["prediction"] == [0.5, 1.5]
    assert same(d["prediction"], np.arange(2) + 0.5)
    assert e.responsibility_cost(prm(), cp, 2.0, ids=[])["best_index"] == -1 and rec.take() == []


def test_responsibility_refusals(eng):
    """each refusal with today's text, bare and with the agent in front, in today's order, before any library call"""
    e, rec = eng
    bad_len, bad_mode = cost_prm(responsibility=3), cost_prm(mode=_abi.FX_RISK_RESP_NONE)
    for pred in ("step", "probability"):      # (the probability pass is a library call as well: none of it either)
        with pytest.raises(ValueError, match="^responsibility has 3 entries for 2 obstacles$"):
            e.responsibility_cost(prm(), bad_len, 0, prediction=pred)                    # (the length before the weight)
        with pytest.raises(ValueError, match="^responsibility weight 0: a non-zero number$"):
            e.responsibility_cost(prm(), bad_mode, 0, prediction=pred)                   # (the weight before the mode)
        with pytest.raises(ValueError, match="^responsibility weight nan: a non-zero number$"):
            e.responsibility_cost(prm(), cost_prm(), float("nan"), prediction=pred)
        with pytest.raises(ValueError, match="^responsibility_mode 0: the action-space factors or 'reach_set'$"):
            e.responsibility_cost(prm(), bad_mode, 1.0, prediction=pred)
        three = lambda cps, w: e.responsibility_cost_batch([prm()] * 3, cps, w, prediction=pred)
        with pytest.raises(ValueError, match="^agent 2: responsibility has 3 entries for 1 obstacles$"):
            three([cost_prm(), cost_prm(), bad_len], [1.0, 1.0, 0.0])
        with pytest.raises(ValueError, match="^agent 1: responsibility weight 0.0: a non-zero number$"):      # (the batch prints the float)
            three([cost_prm(), bad_mode, cost_prm()], [1.0, 0, 1.0])
        with pytest.raises(ValueError, match="^agent 1: responsibility weight nan: a non-zero number$"):
            three([cost_prm()] * 3, [1.0, float("nan"), 1.0])
        with pytest.raises(ValueError, match="^agent 0: responsibility_mode 0: the action-space factors or 'reach_set'$"):
            three([bad_mode, cost_prm(), bad_len], [1.0, 1.0, 1.0])                      # (agent by agent: 0's mode before 2's length)
    with pytest.raises(ValueError, match="^prediction 'x': 'step' or 'probability'$"):
        e.responsibility_cost(prm(), bad_len, 0, prediction="x")
    with pytest.raises(ValueError, match="^prediction 'x': 'step' or 'probability', or one of them per listed agent$"):
        e.responsibility_cost_batch([prm()] * 3, [bad_len] * 3, [0.0] * 3, prediction="x")
    with pytest.raises(ValueError, match="^3 params, 3 cost_params and 2 weights for 3 agents$"):
        e.responsibility_cost_batch([prm()] * 3, [bad_len] * 3, [0.0] * 2)
    assert rec.take() == []


# ---- hypotheses / hypotheses_batch ----
def hypothesis_sets():
    full = dict(K=2, P=3, pos=np.arange(12.0).reshape(2, 3, 2), cov_inv=np.arange(24.0).reshape(2, 3, 4) + 100, npred=np.array([3, 2], np.int32),
                hull=np.arange(24.0).reshape(2, 2, 6) + 200, nhull=np.array([2, 1], np.int32))
    few = dict(K=1, P=2, pos=np.arange(4.0).reshape(1, 2, 2) + 1, cov_inv=np.arange(8.0).reshape(1, 2, 4) + 101, npred=np.array([2], np.int32),
               hull=np.arange(6.0).reshape(1, 1, 6) + 201, nhull=np.array([1], np.int32))
    return full, few


def few_at_2_3():
    """`few` padded with an absent obstacle and re-strided to K = 2, P = 3, written out"""
    pos, cov, hull = np.zeros((2, 3, 2)), np.zeros((2, 3, 4)), np.zeros((2, 2, 6))
    pos[0, :2], cov[0, :2], hull[0, :1] = np.arange(4.0).reshape(2, 2) + 1, np.arange(8.0).reshape(2, 4) + 101, np.arange(6.0) + 201
    return dict(pos=list(pos.ravel()), cov_inv=list(cov.ravel()), npred=[2, 0], hull=list(hull.ravel()), nhull=[1, 0])


def as_lists(s):
    return {k: [x for x in np.asarray(s[k]).ravel()] for k in ("pos", "cov_inv", "npred", "hull", "nhull")}


NULL_HYP = dict(pos=None, cov_inv=None, npred=None, hull=None, nhull=None)


def test_hypotheses(eng):
    e, rec = eng
    full, few = hypothesis_sets()
    one = [e.hypotheses([full, few], agent=0, pred=True, totals=True, collisions=True), e.hypotheses([few], agent=1, pred=True, totals=True, collisions=True),
           e.hypotheses(few, agent=2, pred=True, totals=True, collisions=True)]      # (a bare dict is one set)
    calls = rec.take()
    every = ["winner", "cost", "n_collisions", "pred", "total", "collision"]
    assert calls == [("fx_eval_hypotheses_agent", dict(agent=0, n_hyp=2, hyp=[as_lists(full), few_at_2_3()], bound=every)),
                     ("fx_eval_hypotheses_agent", dict(agent=1, n_hyp=1, hyp=[NULL_HYP], bound=every)),      # (K == 0: the entries stay NULL)
                     ("fx_eval_hypotheses_agent", dict(agent=2, n_hyp=1, hyp=[as_lists(few)], bound=every))]
    for d, h, n in zip(one, (2, 1, 1), N_CAND):
        assert list(d) == ["winner", "cost", "n_collisions", "pred", "totals", "collisions"]
        assert same(d["winner"], np.arange(h)) and same(d["cost"], np.arange(h) + 0.5) and same(d["n_collisions"], np.arange(h) + 10)
        assert same(d["pred"], (np.arange(h * n) + 0.25).reshape(h, n)) and same(d["totals"], (np.arange(h * n) + 0.75).reshape(h, n))
        assert same(d["collisions"], (np.arange(h * n) % 2).astype(bool).reshape(h, n))

    bat = e.hypotheses_batch([[full, few], [few], few], pred=True, totals=True, collisions=True)
    (name, call), = rec.take()
    assert name == "fx_eval_hypotheses_batch" and (call["n"], call["agents"], call["n_hyp"], call["bound"]) == (3, [0, 1, 2], [2, 1, 1], every)
    assert call["hyp"] == [h for c in calls for h in c[1]["hyp"]]      # element for element what the per-agent calls filled
    p0 = c0 = 0
    for d, h, n in zip(bat, (2, 1, 1), N_CAND):
        assert list(d) == ["winner", "cost", "n_collisions", "pred", "totals", "collisions"]
        assert same(d["winner"], np.arange(p0, p0 + h)) and same(d["cost"], np.arange(p0, p0 + h) + 0.5)
        assert same(d["n_collisions"], np.arange(p0, p0 + h) + 10)
        assert same(d["pred"], (np.arange(c0, c0 + h * n) + 0.25).reshape(h, n)) and same(d["totals"], (np.arange(c0, c0 + h * n) + 0.75).reshape(h, n))
        assert same(d["collisions"], (np.arange(c0, c0 + h * n) % 2).astype(bool).reshape(h, n))
        p0, c0 = p0 + h, c0 + h * n
    for k in ("winner", "cost", "n_collisions", "pred", "totals", "collisions"):
        assert one_base([d[k] for d in bat]), k

    # nothing asked for: the blocks are NULL and None; agents in any order
    bat = e.hypotheses_batch([[few], [full]], agents=[2, 0])
    (name, call), = rec.take()
    assert (call["agents"], call["n_hyp"], call["bound"]) == ([2, 0], [1, 1], ["winner", "cost", "n_collisions"])
    assert call["hyp"] == [as_lists(few), as_lists(full)]
    assert all(d["pred"] is None and d["totals"] is None and d["collisions"] is None for d in bat)
    d = e.hypotheses([full])
    assert rec.take()[0][1]["bound"] == ["winner", "cost", "n_collisions"] and d["pred"] is None and d["collisions"] is None
    d = e.hypotheses([], totals=True)      # (no set: the call is the library's to refuse, the answers have one entry)
    assert rec.take() == [("fx_eval_hypotheses_agent", dict(agent=0, n_hyp=0, hyp=[], bound=["winner", "cost", "n_collisions", "total"]))]
    assert d["winner"].shape == (1,) and d["totals"].shape == (1, 5)
    assert e.hypotheses_batch([]) == [] and rec.take() == []

    wrong = dict(full, pos=np.zeros(11))
    with pytest.raises(ValueError, match="^hypothesis array of 11 values, the upload's K=2, P=3 need 12$"):
        e.hypotheses([full, wrong])
    with pytest.raises(ValueError, match="^hypothesis array of 11 values, the upload's K=2, P=3 need 12$"):
        e.hypotheses_batch([[few], [full, wrong]], agents=[2, 0])
    with pytest.raises(ValueError, match="^2 predicted obstacles in a hypothesis for an upload of K=1$"):
        e.hypotheses_batch([[full]], agents=[2])
    with pytest.raises(ValueError, match="^2 lists of prediction sets for 1 agents$"):
        e.hypotheses_batch([[full], [few]], agents=[0])
    assert rec.take() == []
    assert e.last_hypotheses_info == dict(steps_per_item=1, rounds=2, launches=3)


# ---- rescore / rescore_batch ----
def test_rescore(eng):
    e, rec = eng
    w0, w1, w2 = np.arange(6.0).reshape(2, 3) + 1, np.zeros((1, 0)), np.arange(6.0).reshape(3, 2) + 11
    d = e.rescore(w0, totals=True)
    assert rec.take() == [("fx_rescore_agent", dict(agent=0, n_vec=2, w=list(w0.ravel()), totals=True))]
    assert list(d) == ["winner", "cost", "totals"] and same(d["winner"], np.arange(2)) and same(d["totals"], (np.arange(10) + 0.25).reshape(2, 5))
    d = e.rescore(w2[0], agent=2)      # (one vector is one set)
    assert rec.take() == [("fx_rescore_agent", dict(agent=2, n_vec=1, w=[11.0, 12.0], totals=False))] and d["totals"] is None
    row = np.arange(7.0) + 0.125
    w2r = np.arange(9.0).reshape(3, 3) + 21
    d = e.rescore(w2r, agent=2, resp=row)
    assert rec.take() == [("fx_rescore_agent_rows", dict(agent=2, n_vec=3, w=list(w2r.ravel()), totals=False, pred=None, resp=list(row)))]
    assert same(d["winner"], np.arange(3) + 200)
    e.rescore(w2, agent=2, pred=row)
    assert rec.take() == [("fx_rescore_agent_rows", dict(agent=2, n_vec=3, w=list(w2.ravel()), totals=False, pred=list(row), resp=None))]
    with pytest.raises(ValueError, match=r"^pred of shape \(5,\) for 7 candidates$"):
        e.rescore(w2, agent=2, pred=np.zeros(5))

    out = e.rescore_batch([w0, w1, w2])
    assert rec.take() == [("fx_rescore_batch", dict(n=3, agents=[0, 1, 2], n_vec=[2, 1, 3], w=list(w0.ravel()) + list(w2.ravel()),
                                                    pred=None, resp=None))]      # (no agent has a row: NULL tables)
    assert [list(d) for d in out] == [["winner", "cost"]] * 3
    assert [list(d["winner"]) for d in out] == [[0, 1], [2], [3, 4, 5]] and same(out[2]["cost"], np.arange(3, 6) + 0.5)
    assert one_base([d["winner"] for d in out]) and one_base([d["cost"] for d in out])

    w0r, row5 = np.arange(8.0).reshape(2, 4) + 31, np.arange(5.0) + 0.375
    out = e.rescore_batch([w2, w0r], agents=[2, 0], pred=[row, None], resp=[None, row5])
    assert rec.take() == [("fx_rescore_batch", dict(n=2, agents=[2, 0], n_vec=[3, 2], w=list(w2.ravel()) + list(w0r.ravel()),
                                                    pred=[list(row), None], resp=[None, list(row5)]))]
    assert [list(d["winner"]) for d in out] == [[0, 1, 2], [3, 4]]
    e.rescore_batch([w2, w0], agents=[2, 0], pred=[row, None])
    assert rec.take()[0][1]["resp"] is None
    assert e.rescore_batch([]) == []
    with pytest.raises(ValueError, match="^2 weight sets for 1 agents, 2 pred and 2 resp rows$"):
        e.rescore_batch([w0, w2], agents=[0])
    with pytest.raises(ValueError, match=r"^resp of shape \(7,\) for 5 candidates$"):
        e.rescore_batch([w0r], resp=[row])
    assert rec.take() == []


# ---- candidates / materialise / materialise_batch / ranked ----
def assert_rows(d, ids, n_cost, bst):
    ids = np.asarray(ids, np.int64)
    assert list(d) == ["planes", "lon", "lat", "tau_lat", "traj_len", "raw_costs", "cost", "flags", "boundary_step"]
    assert same(d["cost"], ids.astype(np.float64)) and same(d["flags"], ids.astype(np.uint32)) and same(d["traj_len"], ids.astype(np.int32))
    assert d["planes"].shape == (len(ids), _abi.FX_NUM_PLANES, S) and np.array_equal(d["planes"][:, 3, 2], ids)
    assert d["lon"].shape == (len(ids), 6) and d["lat"].shape == (len(ids), 6) and d["tau_lat"].shape == (len(ids),)
    assert np.array_equal(d["lon"][:, 5], ids + 0.05) and np.array_equal(d["lat"][:, 0], ids + 0.06) and np.array_equal(d["tau_lat"], ids + 0.12)
    assert same(d["raw_costs"], 10.0 * ids[:, None] + np.arange(n_cost)[None, :])
    assert d["boundary_step"] is None if not bst else same(d["boundary_step"], ids.astype(np.int32))


def test_candidates_and_materialise(eng):
    e, rec = eng
    d = e.candidates([4, 1, 3, 1])      # unsorted with a duplicate: ascending to the library, the caller's order back
    assert rec.take() == [("fx_read_candidates_agent", dict(agent=0, n=4, ids=[1, 1, 3, 4], null=[]))]
    assert_rows(d, [4, 1, 3, 1], 3, True)
    d = e.candidates([1, 2, 2, 6], agent=2)      # the parts the step did not store: NULL and None
    assert rec.take() == [("fx_read_candidates_agent", dict(agent=2, n=4, ids=[1, 2, 2, 6], null=["planes", "co", "tl", "raw", "bst"]))]
    assert [k for k, v in d.items() if v is None] == ["planes", "lon", "lat", "tau_lat", "traj_len", "raw_costs", "boundary_step"]
    assert same(d["cost"], np.array([1.0, 2.0, 2.0, 6.0]))
    d = e.candidates([6, 2], agent=2)
    assert rec.take()[0][1]["ids"] == [2, 6] and same(d["flags"], np.array([6, 2], np.uint32))

    d = e.materialise([4, 1, 3, 1])      # (a set keeps the caller's order, and every part)
    assert rec.take() == [("fx_materialise_candidates_agent", dict(agent=0, n=4, ids=[4, 1, 3, 1])),
                          ("fx_read_materialised_agent", dict(agent=0, n=4, ids=[4, 1, 3, 1], null=[]))]
    assert_rows(d, [4, 1, 3, 1], 3, True)
    d = e.materialise([6, 2], agent=2)
    assert rec.take()[1] == ("fx_read_materialised_agent", dict(agent=2, n=2, ids=[6, 2], null=["bst"]))
    assert_rows(d, [6, 2], 2, False)

    out = e.materialise_batch([[2, 0], [], [6]])
    calls = rec.take()
    assert calls[0] == ("fx_materialise_candidates_batch", dict(n=3, agents=[0, 1, 2], n_ids=[2, 0, 1], ids=[[2, 0], None, [6]]))
    assert calls[1:] == [("fx_read_materialised_agent", dict(agent=0, n=2, ids=[2, 0], null=[])),
                         ("fx_read_materialised_agent", dict(agent=1, n=0, ids=[], null=["raw", "bst"])),      # (no cost term: no raw rows)
                         ("fx_read_materialised_agent", dict(agent=2, n=1, ids=[6], null=["bst"]))]
    assert_rows(out[0], [2, 0], 3, True)
    assert_rows(out[1], [], 0, False)
    assert_rows(out[2], [6], 2, False)
    out = e.materialise_batch([[6, 6], [1]], agents=[2, 0])
    calls = rec.take()
    assert calls[0] == ("fx_materialise_candidates_batch", dict(n=2, agents=[2, 0], n_ids=[2, 1], ids=[[6, 6], [1]]))
    assert [c[1]["agent"] for c in calls[1:]] == [2, 0]
    assert e.materialise_batch([]) == []
    assert rec.take() == [("fx_materialise_candidates_batch", dict(n=0, agents=None, n_ids=None, ids=None))]
    with pytest.raises(ValueError, match="^2 lists for 1 agents$"):
        e.materialise_batch([[1], [2]], agents=[0])
    with pytest.raises(IndexError):      # (an agent that is not there: before the library is asked)
        e.materialise([1], agent=7)
    assert rec.take() == []
    assert e.last_materialise_info == dict(lanes=1, launches=2, rows=3)


def test_ranked(eng):
    e, rec = eng
    ids, cost, flags = e.ranked(2, 10, with_cost=True)      # the buffers' room is clamped to the agent's candidates, n is not
    assert rec.take() == [("fx_read_ranked_agent", dict(agent=0, first=2, n=10, null=[]))]
    assert (ids.shape, ids.dtype, cost.shape, cost.dtype, flags.shape, flags.dtype) == ((5,), np.int64, (5,), np.float64, (5,), np.uint32)
    ids = e.ranked(0, 3, agent=2)
    assert rec.take() == [("fx_read_ranked_agent", dict(agent=2, first=0, n=3, null=["cost", "flags"]))] and ids.shape == (3,)
    assert e.ranked(0, -4).shape == (0,) and rec.take()[0][1]["n"] == -4
    assert e.ranked(0, 4, agent=7).shape == (0,) and rec.take()[0][1]["agent"] == 7      # (an agent the library will refuse: no room)
