"""Every batched entry point with more agents than a wave has lanes: the batched plan step, fx_read_topk_batch,
fx_sort_candidates_batch, the packaged batch and the batched passes of DESIGN.md sections 18-21, at A = 64, 65 and 129 agents in one
launch -- the last count one ballot of row_of / batch_row_of covers, the first that needs the second, and a third iteration with one
live lane ("Beyond one wave of agents").

Agents: synthetic.make_inputs scenes that cycle over grids of 63, 64, 65 and 130 candidates (a grid (n_t, n_v, n_d) has
n_t n_v (n_d + 1) candidates), default horizon, 2 or 3 obstacles, bundle and cost map written, the default cost list (with
`prediction`); v0, v_des, the reference kind and the seed differ from agent to agent, so no two agents have the same answer.
Agent 0 returns nothing (a lateral start rate no candidate survives); agents 63 and 128 have no risk obstacle (K = 0: rows without
an item, which share item0 with the row behind them); agent a has a road boundary when a % 5 is 0, 3 or 4 (0, 63, 64, 65, 128 do).

Two references per leg: (a) the per-agent call -- for the step, the same problem alone on a one-agent context under the batch's
work decomposition; for the passes beside the step, the per-agent entry on the same context -- bit for bit; (b) for the agents
0, 63, 64 and A - 1 (and their neighbours 62, 65 and A - 2) what the per-agent modules hold their calls to: oracle.plan_step
through compare(), the NumPy restatements, NumPy's lexsort / stable argsort, at those modules' bounds.

Six agents have no winner (every selectable candidate collides); the others' (winner, cost) pairs are pairwise different."""
import functools

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, synthetic
from tests import device_planes as dp
from tests import predprob_restatement as pp
from tests import risk_costs_restatement as rcr
from tests import risk_restatement as rr
from tests.risk_scenes import HARM, MODES, predictions, reach_sets, resp_cost, weight
from tests.risk_scenes import ego as ego_of, err as rel_err
from tests.test_risk_costs_gpu import COLS, WEIGHTS

AGENT_COUNTS = (64, 65, 129)
GRIDS = {63: (3, 3, 6), 64: (4, 4, 3), 65: (1, 13, 4), 130: (13, 5, 1)}
SIZES = (63, 64, 65, 130)
KINDS = ("arc", "straight", "scurve")
NOTHING_RETURNED = 0          # the agent whose step returns no candidate
NO_RISK_OBSTACLE = (63, 128)  # K = 0
NO_WINNER = (0, 2, 7, 10, 37, 61)   # every selectable candidate collides (agent 0: there is none)
KS = (1, 32, 33, 64)
COSTED, NEED = 0x10, 0xB      # NEED: VALID | FEASIBLE | RETURNED
S = 31
RESULT_SKIP = ("kernel_ms",)
PLANES = ("x", "y", "theta", "v")
ROWS = ("ego_risk", "obst_risk", "obst_harm_occ")


def agent_kw(a, boundary=True):
    kw = dict(ref_kind=KINDS[a % 3], v0=6.0 + 0.07 * a, v_des=9.0 + 0.05 * (a % 11), grid=GRIDS[SIZES[a % 4]], n_obstacles=2 + a % 2,
              seed=200 + a, d0=0.2 - 0.01 * (a % 7), obstacle_min_gap=15.0)
    if boundary and a % 5 in (0, 3, 4):
        kw["road_half_width"] = 1.5 + 0.05 * (a % 7)
    if a == NOTHING_RETURNED:
        kw["dd0"] = 8.0
    return kw


def make(a, hull_builder, boundary=True):
    return synthetic.make_inputs(hull_builder=hull_builder, **agent_kw(a, boundary))


def subset_of(A):
    """agents given out of order, across the 64-row boundary"""
    return list(dict.fromkeys(a for a in (A - 1, 64, 0, 63, 65) if a < A))


def risk_K(a):
    """risk obstacles of agent a: light agents in front, heavy ones behind, so that under one scratch limit a round of the agents in
    front holds more than 64 rows and the rounds behind it fewer"""
    if a in NO_RISK_OBSTACLE:
        return 0
    return {0: 2, 64: 3}.get(a, 1 if a < 70 else 3 + a % 2)


def edge_agents(A):
    return sorted({0, 63, 64, A - 1} & set(range(A)))


def reference_agents(A):
    """the agents held to the independent references: the edge agents (one that returns nothing, two without a risk obstacle) and
    their neighbours 62, 65 and A - 2, which have obstacles and candidates to compare"""
    return sorted(set(edge_agents(A)) | {a for a in (62, 65, A - 2) if a < A})


def _hip_hulls():
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return build_obstacle_hulls


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(got, want, what):
    assert np.shape(got) == np.shape(want), (what, np.shape(got), np.shape(want))
    assert np.array_equal(_bits(got), _bits(want)), what


def _same_dict(got, want, what):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            _same_bits(got[k], w, (what, k))
        elif isinstance(w, float):
            assert int(dp.bits(got[k])) == int(dp.bits(w)), (what, k, got[k], w)
        else:
            assert got[k] == w, (what, k, got[k], w)


def _same_package(pa, pb, what):
    assert (pa is None) == (pb is None), what
    if pa is not None:
        assert pa.index == pb.index and pa.cost == pb.cost and pa.flags == pb.flags and pa.traj_len == pb.traj_len, what
        assert np.array_equal(pa.block, pb.block) and np.array_equal(pa.raw_costs, pb.raw_costs), what   # every row of the block
        assert np.array_equal(pa.lon, pb.lon) and np.array_equal(pa.lat, pb.lat) and pa.tau_lat == pb.tau_lat, what


def _same_result(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        if k not in RESULT_SKIP:
            if isinstance(want[k], float):
                assert int(dp.bits(got[k])) == int(dp.bits(want[k])), (what, k, got[k], want[k])
            else:
                assert got[k] == want[k], (what, k, got[k], want[k])


def _pin_key(info):
    return (info["lanes_per_candidate"], info["waves_per_simd"], bool(info["grid_kernel"]), info["block"], info["wave_split"],
            bool(info["obstacle_kernel"]), info["obstacle_steps_per_item"])


def _pin(e, pin):
    """force the work decomposition a batch's step_info reported (tests/test_frame_invariance_gpu.py::_pin_decomposition)"""
    lanes, waves, grid, block, split, obstacle_kernel, per_item = pin
    e.set_tuning(lanes, waves, 2 if grid else 1, block if grid else 0, 0 if lanes == 1 else (2 if split else 1))
    e.set_obstacle_stage(2 if obstacle_kernel else 1, per_item if obstacle_kernel else 0)


def _read_step(e, inp, a, res):
    """what a step leaves of agent a of context e"""
    cost, flags = e.costs(a)
    d = dict(res=res, cost=cost, flags=flags, costmap=e.costmap(a), planes={n: e.plane(n, a) for n in PLANES},
             bsteps=e.boundary_steps(a) if inp.mode & _abi.FX_MODE_ROAD_BOUNDARY else None,
             package=e.package(a, 0.01 * a) if e.packaging else None)
    return d


def _same_step(got, want, what):
    """two read-backs of _read_step: result, costs and flags and boundary steps of every candidate, the cost map and the planes of
    the stored ones -- bit for bit"""
    _same_result(got["res"], want["res"], what)
    _same_bits(got["cost"], want["cost"], (what, "cost"))
    assert np.array_equal(got["flags"], want["flags"]), what
    stored = (got["flags"] & COSTED) != 0
    _same_bits(got["costmap"][stored], want["costmap"][stored], (what, "costmap"))
    assert (got["bsteps"] is None) == (want["bsteps"] is None), what
    if got["bsteps"] is not None:
        assert np.array_equal(got["bsteps"], want["bsteps"]), (what, "boundary_steps")
    for n in PLANES:
        _same_bits(got["planes"][n][:, stored], want["planes"][n][:, stored], (what, n))


@functools.lru_cache(maxsize=None)
def solo_steps(pin, boundary=True):
    """(a) for the step: every one of the 129 agents alone on a one-agent context under the decomposition `pin` -- the step, its
    read-back, the top-k at every k, the sort with its ranks, the package.  Computed once per decomposition, left unchanged."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    lanes, waves, grid, block, split, obstacle_kernel, per_item = pin
    out = []
    with FrenetEngine(max_candidates=256, max_agents=1) as e:
        e.set_package(True)
        _pin(e, pin)
        for a in range(max(AGENT_COUNTS)):
            inp = make(a, _hip_hulls(), boundary)
            res = e.plan_step(inp)
            one = e.step_info()
            assert one["agents"] == 1 and not one["step_kernel"], one
            assert (one["lanes_per_candidate"], bool(one["grid_kernel"]), one["wave_split"]) == (lanes, grid, split), (a, one, pin)
            assert bool(one["obstacle_kernel"]) == obstacle_kernel, (a, one, pin)
            d = _read_step(e, inp, 0, res)
            d["topk"] = {k: tuple(x[0].copy() for x in e.topk(k)) for k in KS}
            n_pool, n_nan = e.sort_candidates(0)
            d["sort"] = (n_pool, n_nan) + (e.ranked(0, n_pool, 0, with_cost=True) if n_pool else ())
            d["package"] = e.package(0, 0.01 * a)
            out.append(d)
    return out


def _scene(eng, a, inp, src=None):
    """agent a's K = risk_K(a) risk obstacles along its own candidates (tests/test_resp_batch_gpu.py::_scene; `src`: the planes and
    flags of another agent for the one that returned nothing), reach sets and the action-space vector, set on the engine"""
    from frenetix_motion_planner_amd import risk
    _, flags = eng.costs(a)
    planes = {n: eng.plane(n, a).T.copy() for n in PLANES}
    walk_planes, walk_flags = (planes, flags) if src is None else src
    K, modes = risk_K(a), MODES[a % 5]
    maha = bool(modes.get("fast_prob_mahalanobis"))
    preds, typ = predictions(walk_planes, walk_flags, np.random.default_rng(1000 + a), n_obs=K, zero_cov=not maha) if K else ({}, {})
    keys = list(preds)
    ok = np.nonzero((walk_flags & NEED) == NEED)[0]
    x0 = np.array([walk_planes["x"][ok[0], 0], walk_planes["y"][ok[0], 0]])
    th0 = float(walk_planes["theta"][ok[0], 0]) + 0.5
    sets = reach_sets(walk_planes, keys, ok[::3], inp.dt) if K else {}
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ, mahalanobis=maha), a)
    eng.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples), a)
    vec = risk.action_space_responsibility(preds, x0, th0)
    reach = a % 2 == 0
    return dict(flags=flags, planes=planes, preds=preds, typ=typ, keys=keys, sets=sets, vec=vec, x0=x0, th0=th0, modes=modes, K=K,
                params=risk.risk_params(modes, HARM, **ego_of(a)), cost=resp_cost("reach_set" if reach else vec),
                cost_other=resp_cost(vec if reach else "reach_set"), reach=reach, weight=weight(a))


def _cp(**kw):
    from frenetix_motion_planner_amd import risk
    return risk.risk_cost_params(WEIGHTS, **kw)


def list_form(a):
    """the list form of agent a: 0 none / 1 one id / 2 descending ids with gaps / 3 an empty list / 4 all.  Agents 63, 64 and 65:
    none, one id, descending -- so the agents without a risk obstacle, 63 and 128, have rows with candidates and no item in the
    listed calls too.  An empty list makes no row at all: only agents from 65 on have one (below, "all" stands in), so that a call
    over 65 agents has 65 rows and is the first to need the second ballot."""
    form = (a + 2) % 5
    return 4 if form == 3 and a < 65 else form


def _lists(scenes):
    """the mixed list forms of tests/test_risk_batch_gpu.py by list_form: none / one id / descending ids with gaps (65 of them on an
    agent of 130 candidates) / an empty list / all"""
    out = []
    for a, sc in enumerate(scenes):
        n = len(sc["flags"])
        form = list_form(a)
        if form == 0:
            out.append(None)
        elif form == 1:
            out.append(np.array([(7 * a) % n]))
        elif form == 2:
            out.append(np.arange(n - 1, -1, -2)[:65].copy())
        elif form == 3:
            out.append(np.zeros(0, np.int64))
        else:
            out.append(np.arange(n))
    assert any(x is not None and len(x) == 65 for x in out)
    return out


def _cost_forms(scenes):
    """(lists, cost parameters) of the detail / cost call: the lists of _lists, but "all" is the list the min_risk_cost fallback
    makes (every VALID & FEASIBLE & RETURNED candidate); by a % 3 the detail alone / reach-set responsibility / the action-space
    vector with a boundary array"""
    lists, costs = _lists(scenes), []
    for a, sc in enumerate(scenes):
        if list_form(a) == 4:
            lists[a] = np.nonzero((sc["flags"] & NEED) == NEED)[0]
        n = len(sc["flags"]) if lists[a] is None else len(lists[a])
        if a % 3 == 0:
            costs.append(None)
        elif a % 3 == 1:
            costs.append(_cp(responsibility="reach_set"))
        else:
            costs.append(_cp(boundary_harm=np.where(np.arange(n) % 3 == 0, 0.0, np.linspace(0.05, 0.45, n)), responsibility=sc["vec"]))
    return lists, costs


class Batch:
    """one context of A agents behind one batched plan step, with everything the tests compare -- computed once, left unchanged"""

    def __init__(self, A):
        from frenetix_motion_planner_amd.engine import FrenetEngine
        self.A = A
        self.inps = [make(a, _hip_hulls()) for a in range(A)]
        assert [i.n_candidates for i in self.inps] == [SIZES[a % 4] for a in range(A)] and {i.n_samples for i in self.inps} == {S}
        assert all("prediction" in i.cost_names and i.write_bundle and i.write_costmap for i in self.inps)
        self.eng = e = FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in self.inps), max_agents=A)
        e.set_package(True)
        self.res = e.plan_batch(self.inps)
        self.info = e.step_info()
        self.step = [_read_step(e, self.inps[a], a, self.res[a]) for a in range(A)]
        self.topk = {k: e.topk(k) for k in KS}
        self.n_pool, self.n_nan = e.sort_candidates_batch()
        self.ranked = [e.ranked(0, int(self.n_pool[a]), a, with_cost=True) if self.n_pool[a] else () for a in range(A)]
        self.solo = solo_steps(_pin_key(self.info))[:A]
        src = None
        self.scenes = [None] * A
        for a in list(range(1, A)) + [0]:      # (agent 0 returned nothing: its obstacles walk along agent 1's candidates)
            self.scenes[a] = _scene(e, a, self.inps[a], src if a == NOTHING_RETURNED else None)
            if a == 1:
                src = (self.scenes[1]["planes"], self.scenes[1]["flags"])
        self.ln = [ego_of(a)["ego_length"] for a in range(A)]
        self.wd = [ego_of(a)["ego_width"] for a in range(A)]

    def close(self):
        self.eng.close()


@pytest.fixture(scope="module", params=AGENT_COUNTS, ids=lambda A: f"A{A}")
def ctx(request):
    b = Batch(request.param)
    yield b
    b.close()


def test_scenes_differ_on_the_oracle():
    """(no GPU) the scenes as they were fixed: no two of the 123 agents with a winner share (winner, winner's cost) and the six
    without one are none of 62 ... 65, 127 and 128; agent 0 returns nothing"""
    from oracle import oracle
    outs = [oracle.plan_step(make(a, oracle.build_obstacle_hulls), want_planes=False) for a in range(max(AGENT_COUNTS))]
    keys = [(o["result"]["best_index"], o["result"]["best_cost"], o["result"]["n_collisions"]) for o in outs]
    assert outs[NOTHING_RETURNED]["returned"].sum() == 0 and keys[NOTHING_RETURNED][0] == -1
    assert tuple(a for a, k in enumerate(keys) if k[0] < 0) == NO_WINNER
    assert len({k[:2] for k in keys if k[0] >= 0}) == len(keys) - len(NO_WINNER)
    assert not set(NO_WINNER) & {62, 63, 64, 65, 127, 128}
    assert sum(k[0] >= 0 and k[2] > 0 for k in keys) >= 6      # (winners with colliding candidates ordered in front of them)
    # candidates off the road and colliding ones in an eighth of the agents of every batch; top-k rows that end before 32, between
    # 33 and 64 and beyond 64 eligible candidates
    eligible = [int(dp.eligible(o["cost"], o["flags"]).sum()) for o in outs]
    for A in AGENT_COUNTS:
        assert sum((o["flags"] & _abi.FX_FLAG_BOUNDARY).any() for o in outs[:A]) > A // 8
        assert sum((o["flags"] & _abi.FX_FLAG_COLLISION).any() for o in outs[:A]) > A // 8
        assert sum(n < 32 for n in eligible[:A]) > 4 and sum(33 <= n < 64 for n in eligible[:A]) > 4 and sum(n > 64 for n in eligible[:A]) > 2


gpu = pytest.mark.gpu


@gpu
def test_agents_differ(ctx):
    """up front: winner index or winner cost differs between the agents 62 / 63 / 64 / 65 and between A - 2 / A - 1 (all agents
    with a winner, in fact), so a row mix-up shows; the edge agents are what the module says of them"""
    A, res = ctx.A, ctx.res
    keys = [(r["best_index"], int(dp.bits(r["best_cost"])), r["n_collisions"]) for r in res]
    assert len({k[:2] for k in keys if k[0] >= 0}) == A - sum(a < A for a in NO_WINNER)
    around = [a for a in (62, 63, 64, 65) if a < A]
    assert len({keys[a] for a in around}) == len(around) and keys[A - 2] != keys[A - 1]
    assert ctx.info["agents"] == A and not ctx.info["step_kernel"], ctx.info      # (set_step_kernel is left alone)
    f0 = ctx.step[NOTHING_RETURNED]["flags"]
    assert not (f0 & _abi.FX_FLAG_RETURNED).any() and res[NOTHING_RETURNED]["best_index"] == -1 and res[NOTHING_RETURNED]["n_returned"] == 0
    assert tuple(a for a, r in enumerate(res) if r["best_index"] < 0) == tuple(a for a in NO_WINNER if a < A)
    assert [ctx.scenes[a]["K"] for a in NO_RISK_OBSTACLE if a < A] == [0] * sum(a < A for a in NO_RISK_OBSTACLE)
    assert all(ctx.inps[a].mode & _abi.FX_MODE_ROAD_BOUNDARY for a in edge_agents(A))
    assert any(not (i.mode & _abi.FX_MODE_ROAD_BOUNDARY) for i in ctx.inps)


# ------------------------------------------------------------------------------------------------------------------ the step
@gpu
def test_plan_step_equals_agents_alone(ctx):
    """result (best index, best cost, collisions, counters, reason histogram), costs and flags, cost map, boundary steps and the
    planes x, y, theta, v of every agent: bit for bit the agent alone under the batch's decomposition"""
    for a in range(ctx.A):
        got, want = ctx.step[a], ctx.solo[a]
        _same_step(got, want, a)
        dp_w, dp_c, dp_n, _ = dp.expected_selection(got["cost"], got["flags"])
        assert (got["res"]["best_index"], got["res"]["n_collisions"]) == (dp_w, dp_n), a
    assert sum((ctx.step[a]["flags"] & _abi.FX_FLAG_COLLISION).any() for a in range(ctx.A)) > ctx.A // 8
    assert sum((ctx.step[a]["flags"] & _abi.FX_FLAG_BOUNDARY).any() for a in range(ctx.A)) > ctx.A // 8


@gpu
def test_plan_step_matches_the_oracle(ctx):
    """(b) the agents 0, 63, 64 and A - 1 of the batch and their neighbours through compare(): decisions exact, costs 1e-9"""
    from oracle import oracle
    from tests.test_hip_parity import compare
    for a in reference_agents(ctx.A):
        ref_inp = make(a, oracle.build_obstacle_hulls)
        compare(ctx.eng, ctx.inps[a], oracle.plan_step(ref_inp), ctx.res[a], agent=a, ref_inp=ref_inp)


@gpu
@pytest.mark.parametrize("stage", [1, 2], ids=["obstacles_in_the_walk", "obstacle_kernel"])
def test_split_step_launches(ctx, stage):
    """The batch's own choice for agents this small is one launch with the selection inside (step_info of test_agents_differ), so
    the launches with grid.y = A behind it are reached through the switches the batch modules already use: set_fused_selection(0)
    -- fx_select_kernel ends the step; at 32 slices, 65 agents are the first count beyond 2 048 workgroups -- and
    set_obstacle_stage(2) -- fx_obstacle_kernel between the two, which takes no agent with a road boundary: that leg runs the scenes
    without theirs.  Every agent's step, top-k rows and package equal the agent alone under the decomposition this batch reports."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    A, boundary = ctx.A, stage == 1
    inps = ctx.inps if boundary else [make(a, _hip_hulls(), False) for a in range(A)]
    with FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in ctx.inps), max_agents=A) as e:
        e.set_package(True)
        e.set_fused_selection(0)
        e.set_obstacle_stage(stage)
        res = e.plan_batch(inps)
        info = e.step_info()
        print(f"A = {A}, stage {stage}: {info}")
        assert info["agents"] == A and not info["fused_selection"] and not info["step_kernel"], info
        assert bool(info["obstacle_kernel"]) == (stage == 2), info
        solo = solo_steps(_pin_key(info), boundary)
        for a in range(A):
            _same_step(_read_step(e, inps[a], a, res[a]), solo[a], (stage, a))
            _same_package(e.package(a, 0.01 * a), solo[a]["package"], (stage, a))
            if boundary:
                assert (res[a]["best_index"], res[a]["n_collisions"]) == (ctx.res[a]["best_index"], ctx.res[a]["n_collisions"]), (stage, a)
            assert (res[a]["best_index"], res[a]["n_collisions"]) == dp.expected_selection(*e.costs(a))[0:3:2], (stage, a)
        for k in (1, 64):
            cost, idx = e.topk(k)
            for a in range(A):
                assert np.array_equal(idx[a], solo[a]["topk"][k][1]), (stage, a, k)
                _same_bits(cost[a], solo[a]["topk"][k][0], (stage, a, k))


@gpu
def test_state_update_equals_fresh_uploads(ctx):
    """a second step behind update_state on the agents 63, 64 and A - 1 alone (tests/test_update_paths_gpu.py): what a fresh upload
    of the moved agents leaves, for EVERY agent of the batch"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from tests.test_update_paths_gpu import _agent_update, make_update
    A = ctx.A
    cap = sum(i.n_candidates + 64 for i in ctx.inps)
    moved = sorted({63, 64, A - 1} & set(range(A)))
    twins = list(ctx.inps)
    with FrenetEngine(max_candidates=cap, max_agents=A) as e, FrenetEngine(max_candidates=cap, max_agents=A) as fresh:
        e.upload(ctx.inps)
        e.evaluate()
        first = e.finish()
        for a in range(A):
            _same_result(first[a], ctx.res[a], ("first step", a))
        for a in moved:
            twins[a], fields = _agent_update(ctx.inps[a], 1)
            e.update_state(make_update(twins[a], fields), agent=a)
        e.evaluate()
        ra = e.finish()
        fresh.upload(twins)
        fresh.evaluate()
        rb = fresh.finish()
        assert e.step_info()["agents"] == fresh.step_info()["agents"] == A and not e.step_info()["step_kernel"]
        for a in range(A):
            _same_step(_read_step(e, twins[a], a, ra[a]), _read_step(fresh, twins[a], a, rb[a]), ("update", moved, a))
        for a in moved:
            assert ra[a]["best_cost"] != ctx.res[a]["best_cost"], a      # (the update did move the agent's answer)
        for a in set(range(A)) - set(moved):
            _same_result(ra[a], ctx.res[a], ("an agent that was not moved", a))


@gpu
@pytest.mark.parametrize("k", KS)
def test_topk(ctx, k):
    """fx_read_topk_batch: every agent's row equals the agent's own topk(k) alone and NumPy's lexsort of its cost / flag planes"""
    cost, idx = ctx.topk[k]
    assert cost.shape == idx.shape == (ctx.A, k)
    for a in range(ctx.A):
        wi, wc = ctx.solo[a]["topk"][k][1], ctx.solo[a]["topk"][k][0]
        assert np.array_equal(idx[a], wi), (a, k)
        _same_bits(cost[a], wc, (a, k))
        ni, nc = dp.expected_topk(ctx.step[a]["cost"], ctx.step[a]["flags"], k)
        assert np.array_equal(idx[a], ni), (a, k)
        _same_bits(cost[a], nc, (a, k, "lexsort"))
    assert np.array_equal(idx[:, 0], [r["best_index"] for r in ctx.res])
    assert (idx[:, k - 1] >= 0).sum() > 2 and (k == 1 or (idx[:, k - 1] < 0).sum() > 2)      # (full rows and short ones at every k)


@gpu
def test_sort(ctx):
    """sort_candidates_batch + ranked(0, n_pool, agent) with costs: the agent's own sort alone, and np.argsort(kind="stable") on
    the agent's own costs()"""
    for a in range(ctx.A):
        cost, flags = ctx.step[a]["cost"], ctx.step[a]["flags"]
        pool = np.nonzero((flags & COSTED) == COSTED)[0]
        order = pool[np.argsort(cost[pool], kind="stable")]
        assert (int(ctx.n_pool[a]), int(ctx.n_nan[a])) == (len(pool), int(np.isnan(cost[pool]).sum())) == ctx.solo[a]["sort"][:2], a
        if len(pool):
            ids, c, f = ctx.ranked[a]
            sids, sc, sf = ctx.solo[a]["sort"][2:]
            assert np.array_equal(ids, sids) and np.array_equal(f, sf), a
            _same_bits(c, sc, a)
            assert np.array_equal(ids, order) and np.array_equal(f, flags[order]), a
            _same_bits(c, cost[order], (a, "argsort"))
    assert ctx.n_pool[NOTHING_RETURNED] == 0 and (ctx.n_pool > 0).sum() == ctx.A - 1


@gpu
def test_packages(ctx):
    """the package of every agent behind plan_batch, plan_batch_packaged and plan_batch_begin / plan_batch_end: every row of the
    block and the scalar fields of the agent's own package() alone"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    A = ctx.A
    yaw = [0.01 * a for a in range(A)]
    cap = sum(i.n_candidates + 64 for i in ctx.inps)
    for a in range(A):
        _same_package(ctx.step[a]["package"], ctx.solo[a]["package"], ("plan_batch", a))
    assert [d["package"] is None for d in ctx.step] == [a in NO_WINNER for a in range(A)]
    for a in edge_agents(A):      # (b) the package is the read-back of the winner
        pkg = ctx.step[a]["package"]
        if pkg is not None:
            cand = ctx.eng.candidate(ctx.res[a]["best_index"], a)
            assert pkg.index == ctx.res[a]["best_index"] and pkg.cost == cand["cost"] and pkg.flags == cand["flags"]
            assert np.array_equal(pkg.planes, cand["planes"]) and np.array_equal(pkg.raw_costs, cand["raw_costs"])
    with FrenetEngine(max_candidates=cap, max_agents=A) as e:
        inps = [make(a, _hip_hulls()) for a in range(A)]
        res, pk = e.plan_batch_packaged(inps, yaw)
        assert e.step_info()["agents"] == A and not e.step_info()["step_kernel"]
        for a in range(A):
            _same_result(res[a], ctx.res[a], ("packaged", a))
            _same_package(pk[a], ctx.solo[a]["package"], ("packaged", a))
        res, pk = e.plan_batch_packaged(inps, yaw)      # (the same structures: every agent updated in place)
        for a in range(A):
            _same_result(res[a], ctx.res[a], ("packaged, in place", a))
            _same_package(pk[a], ctx.solo[a]["package"], ("packaged, in place", a))
    with FrenetEngine(max_candidates=cap, max_agents=A) as e:
        tok = e.plan_batch_begin(inps)
        assert tok is not None
        res, pk = e.plan_batch_end(tok, yaw)
        for a in range(A):
            _same_result(res[a], ctx.res[a], ("begin / end", a))
            _same_package(pk[a], ctx.solo[a]["package"], ("begin / end", a))


# ------------------------------------------------------------------------------------------- rounds of the passes beside the step
def _rounds(agents, limit):
    """rows per round of a call: the statement of fx_item_rounds (csrc/fx_pass.h) over agents [(n, bytes per candidate)] -- a round
    is closed when the next tile of 64 does not fit; an agent has one row in every round it has a tile in"""
    rows, cur, used = [], set(), 0
    for a, (n, per) in enumerate(agents):
        for _ in range(0, n, 64):
            if used > 0 and 64 * per > limit - min(used, limit):
                rows.append(len(cur))
                cur, used = set(), 0
            cur.add(a)
            used += 64 * per
    return rows + ([len(cur)] if cur else [])


def _limit(agents, A):
    """the scratch limit of the forced rounds: what the tiles of the agents in front take -- of the first 67 agents with a row at
    129 (a round of more than 64 rows; the heavy agents behind take several rounds of fewer), of the first 21 otherwise -- checked
    on _rounds"""
    with_row = np.nonzero([n > 0 for n, _ in agents])[0]
    upto = int(with_row[66 if A == 129 else 20]) + 1
    limit = sum(-(-n // 64) * 64 * per for n, per in agents[:upto])
    rows = _rounds(agents, limit)
    assert len(rows) >= 3 and min(rows) < 64 and (max(rows) > 64) == (A == 129), (A, limit, rows)
    assert _rounds(agents, 64 << 20) in ([len([1 for n, _ in agents if n > 0])], [])
    return limit, rows


def _item_share(lib, n, K, doubles):
    return 8 * doubles * K * -(-(S - 1) // lib.fx_risk_items_chunk_steps(n, S, K)) if K and n else 0


# ----------------------------------------------------------------------------------------------------- prediction probability
def _pp_same(got, want, what):
    _same_dict(got, want, what)


@gpu
@pytest.mark.parametrize("rounds", ["one", "forced"])
def test_prediction_probability_batch(ctx, rounds):
    from frenetix_motion_planner_amd._lib import lib
    e, A = ctx.eng, ctx.A
    solo = [e.prediction_probability(ctx.ln[a], ctx.wd[a], agent=a) for a in range(A)]
    step = [e.prediction_probability(ctx.ln[a], ctx.wd[a], agent=a, source="step") for a in range(A)]
    agents = [(SIZES[a % 4], 8 * ctx.scenes[a]["K"] * (S - 1)) for a in range(A)]
    subset = subset_of(A)
    if rounds == "forced":
        limit, rows = _limit(agents, A)
        print(f"A = {A}: limit {limit} bytes, rows per round {rows}")
        lib().fx_predprob_set_scratch_limit(limit)
    try:
        got = e.prediction_probability_batch(ctx.ln, ctx.wd)
        some = e.prediction_probability_batch([ctx.ln[a] for a in subset], [ctx.wd[a] for a in subset], agents=subset)
        from_step = e.prediction_probability_batch(ctx.ln, ctx.wd, source="step")
    finally:
        lib().fx_predprob_set_scratch_limit(0)
    assert len(got) == len(from_step) == A and len(some) == len(subset)
    for a in range(A):
        _pp_same(got[a], solo[a], (rounds, a))
        _pp_same(from_step[a], step[a], (rounds, "step", a))
        ids = np.nonzero(ctx.step[a]["flags"] & COSTED)[0]
        assert np.array_equal(from_step[a]["total"][ids], ctx.step[a]["cost"][ids]), a      # source "step": the step's own cost
        assert got[a]["best_index"] == pp.best_index(got[a]["total"], ctx.step[a]["flags"]), a
    for r, a in zip(some, subset):
        _pp_same(r, solo[a], (rounds, subset, a))
    winners = [(r["best_index"], int(dp.bits(r["best_cost"]))) for r in got if r["best_index"] >= 0]
    assert len(set(winners)) == len(winners) > A - 10
    assert sum(np.nansum(r["prob"] > 0) > 0 for r in got) > A // 2
    for a in reference_agents(A):      # (b)
        sc, K = ctx.scenes[a], ctx.scenes[a]["K"]
        ids = np.nonzero(sc["flags"] & COSTED)[0]
        if K == 0 or len(ids) == 0:
            assert np.all(got[a]["prob"][ids] == 0.0) and np.all(np.isnan(np.delete(got[a]["prob"], ids))), a
            continue
        want, _, _ = pp.prediction_probability(sc["planes"]["x"][ids], sc["planes"]["y"][ids], sc["planes"]["theta"][ids], sc["preds"],
                                               ctx.ln[a], ctx.wd[a])
        err = float(np.abs(got[a]["prob"][ids] - want).max())
        print(f"agent {a}: K = {K}, {len(ids)} costed, {int((want > 0).sum())} with a positive sum, error {err:.3e}")
        assert err <= (K * (S - 1) + 1) * 1e-12 and (want > 0).any(), a


# ------------------------------------------------------------------------------------------------------------- responsibility
RESP_KEYS = ("resp", "total", "ego_risk", "obst_risk")


def _resp_same(got, want, what):
    for k in RESP_KEYS:
        _same_bits(got[k], want[k], (what, k))
    assert got["best_index"] == want["best_index"] and int(dp.bits(got["best_cost"])) == int(dp.bits(want["best_cost"])), what


@gpu
@pytest.mark.parametrize("rounds", ["one", "forced"])
def test_responsibility_cost_batch(ctx, rounds):
    """every agent in its own mode (reach sets for even agents, the action-space vector for odd ones), then every agent in the other"""
    from frenetix_motion_planner_amd._lib import lib
    e, A, L = ctx.eng, ctx.A, lib()
    prm, wts = [sc["params"] for sc in ctx.scenes], [sc["weight"] for sc in ctx.scenes]
    agents = [(SIZES[a % 4], _item_share(L, SIZES[a % 4], ctx.scenes[a]["K"], 7)) for a in range(A)]
    subset = subset_of(A)
    for which in ("cost", "cost_other"):
        cps = [sc[which] for sc in ctx.scenes]
        solo = [e.responsibility_cost(prm[a], cps[a], wts[a], agent=a) for a in range(A)]
        if rounds == "forced":
            limit, rows = _limit(agents, A)
            print(f"A = {A}: limit {limit} bytes, rows per round {rows}")
            L.fx_risk_batch_set_scratch_limit(limit)
        try:
            got = e.responsibility_cost_batch(prm, cps, wts)
            some = e.responsibility_cost_batch([prm[a] for a in subset], [cps[a] for a in subset], [wts[a] for a in subset], agents=subset)
        finally:
            L.fx_risk_batch_set_scratch_limit(0)
        assert len(got) == A
        for a in range(A):
            _resp_same(got[a], solo[a], (rounds, which, a))
            assert got[a]["best_index"] == pp.best_index(got[a]["total"], ctx.step[a]["flags"]), a
        for r, a in zip(some, subset):
            _resp_same(r, solo[a], (rounds, which, subset, a))
        assert sum(np.nansum(r["resp"] != 0) > 0 for r in got) > A // 4
        for a in reference_agents(A):      # (b)
            sc, K = ctx.scenes[a], ctx.scenes[a]["K"]
            ids = np.nonzero(sc["flags"] & COSTED)[0]
            if K == 0 or len(ids) == 0:
                assert np.all(got[a]["resp"][ids] == 0.0), a
                continue
            reach = sc["reach"] == (which == "cost")
            P = [sc["planes"][n][ids] for n in PLANES]
            want = rcr.calc_risk_detail(*P, sc["preds"], sc["typ"], sc["modes"], HARM, **ego_of(a))
            if reach:
                wr = [rcr.responsibility_reach_set(P[0][c], P[1][c], ctx.inps[a].dt, sc["sets"], want["obst_risk_max"][c], sc["keys"])[0]
                      for c in range(len(ids))]
            else:
                wr = [rcr.responsibility_action_space(want["obst_risk_max"][c], sc["preds"], sc["x0"], sc["th0"]) for c in range(len(ids))]
            err = rel_err(got[a]["resp"][ids], np.asarray(wr, np.float64))
            print(f"agent {a} ({'reach sets' if reach else 'action space'}): K = {K}, resp error {err:.2e}")
            assert err < (2 * K + 1) * 1e-12, a
            assert rel_err(got[a]["ego_risk"][ids], want["ego_risk"]) < 1e-12 and rel_err(got[a]["obst_risk"][ids], want["obst_risk"]) < 1e-12


# ----------------------------------------------------------------------------------------------------------------------- risk
def _risk_same(got, want, what):
    _same_bits(got[0], want[0], (what, "ego_risk"))
    _same_bits(got[1], want[1], (what, "obst_risk"))
    assert got[2] == want[2], (what, "min_risk_index", got[2], want[2])


@gpu
@pytest.mark.parametrize("rounds", ["one", "forced"])
def test_risk_batch(ctx, rounds):
    from frenetix_motion_planner_amd._lib import lib
    e, A, L = ctx.eng, ctx.A, lib()
    prm = [sc["params"] for sc in ctx.scenes]
    lists = _lists(ctx.scenes)
    assert [None if x is None else len(x) for x in lists[63:66]] == [None, 1, 32][:A - 63]
    assert sum(x is None or len(x) > 0 for x in lists) == (A if A <= 65 else A - 13)      # (rows of the listed call)
    n_of = [SIZES[a % 4] if lists[a] is None else len(lists[a]) for a in range(A)]
    agents = [(n_of[a], _item_share(L, n_of[a], ctx.scenes[a]["K"], 2)) for a in range(A)]
    solo = [e.risk(prm[a], lists[a], agent=a) for a in range(A)]
    subset = subset_of(A)
    if rounds == "forced":
        limit, rows = _limit(agents, A)
        print(f"A = {A}: limit {limit} bytes, rows per round {rows}")
        L.fx_risk_batch_set_scratch_limit(limit)
    try:
        got = e.risk_batch(prm, lists)
        some = e.risk_batch([prm[a] for a in subset], [lists[a] for a in subset], agents=subset)
        whole = e.risk_batch(prm)      # (no agent has a list: the n_ids == NULL form)
    finally:
        L.fx_risk_batch_set_scratch_limit(0)
    assert len(got) == len(whole) == A
    for a in range(A):
        _risk_same(got[a], solo[a], (rounds, a))
        assert got[a][0].shape == (n_of[a],)
    for r, a in zip(some, subset):
        _risk_same(r, solo[a], (rounds, subset, a))
    for a in edge_agents(A) + [a for a in (62, 65) if a < A]:
        _risk_same(whole[a], e.risk(prm[a], None, agent=a), (rounds, "no lists", a))
    for a in (a for a in range(A) if list_form(a) == 3):      # an empty list: no rows, no winner
        assert got[a][2] == -1 and got[a][0].shape == (0,), a
    for a in (a for a in NO_RISK_OBSTACLE if a < A):          # no risk obstacle: rows, no item, every selected risk 0.0
        assert got[a][0].shape == (SIZES[a % 4],) and np.all(got[a][0][(ctx.scenes[a]["flags"] & NEED) == NEED] == 0.0), a
    assert sum((r[0] > 0).any() for r in got) > A // 3
    for a in reference_agents(A):      # (b) on the agent's whole-candidate form
        sc = ctx.scenes[a]
        sel = np.nonzero((sc["flags"] & NEED) == NEED)[0]
        ego, obst, idx = whole[a]
        assert np.all(np.isnan(np.delete(ego, sel))) and not np.isnan(ego[sel]).any(), a
        if len(sel) == 0:
            assert idx == -1
            continue
        P = [sc["planes"][n][sel] for n in PLANES]
        we, wo = rr.calc_risk(*P, sc["preds"], sc["typ"], sc["modes"], HARM, **ego_of(a))
        errs = [rel_err(ego[sel], we), rel_err(obst[sel], wo)]
        print(f"agent {a}: K = {sc['K']}, {len(sel)} candidates, {int((we > 0).sum())} with a risk, errors {errs[0]:.2e} / {errs[1]:.2e}")
        assert max(errs) < 1e-12 and idx == rr.min_risk_index(ego[sel], obst[sel], sel), a


# ---------------------------------------------------------------------------------------------------- risk detail, risk costs
def _solo_costs(e, sc, a, ids, cost):
    return e.risk_detail(sc["params"], ids, agent=a) if cost is None else e.risk_costs(sc["params"], cost, ids, agent=a)


@gpu
@pytest.mark.parametrize("rounds", ["one", "forced"])
def test_risk_detail_and_costs_batch(ctx, rounds):
    from frenetix_motion_planner_amd._lib import lib
    e, A, L = ctx.eng, ctx.A, lib()
    prm = [sc["params"] for sc in ctx.scenes]
    lists, costs = _cost_forms(ctx.scenes)
    n_of = [SIZES[a % 4] if lists[a] is None else len(lists[a]) for a in range(A)]
    agents = [(n_of[a], _item_share(L, n_of[a], ctx.scenes[a]["K"], 7)) for a in range(A)]
    solo = [_solo_costs(e, ctx.scenes[a], a, lists[a], costs[a]) for a in range(A)]
    detail = [_solo_costs(e, ctx.scenes[a], a, lists[a], None) for a in range(A)]
    subset = subset_of(A)
    e.risk_costs_batch(prm, costs, lists)
    assert e.last_risk_costs_batch_rounds == 1
    want_rounds = 1
    if rounds == "forced":
        limit, rows = _limit(agents, A)
        want_rounds = len(rows)
        print(f"A = {A}: limit {limit} bytes, rows per round {rows}")
        L.fx_risk_batch_set_scratch_limit(limit)
    try:
        got = e.risk_costs_batch(prm, costs, lists)
        n_rounds = e.last_risk_costs_batch_rounds
        some = e.risk_costs_batch([prm[a] for a in subset], [costs[a] for a in subset], [lists[a] for a in subset], agents=subset)
        got_detail = e.risk_detail_batch(prm, lists)
    finally:
        L.fx_risk_batch_set_scratch_limit(0)
    assert n_rounds == want_rounds and (rounds == "one" or n_rounds >= 3), (n_rounds, want_rounds)
    assert len(got) == len(got_detail) == A
    for a in range(A):
        _same_dict(got[a], solo[a], (rounds, a))
        _same_dict(got_detail[a], detail[a], (rounds, "detail", a))
        assert ("total" in got[a]) == (costs[a] is not None) and got[a]["ego_risk_max"].shape == (n_of[a], ctx.scenes[a]["K"]), a
    for r, a in zip(some, subset):
        _same_dict(r, solo[a], (rounds, subset, a))
    assert sum("total" in r and np.nansum(r["total"] > 0) > 0 for r in got) > A // 4
    for a in reference_agents(A):      # (b) the detail of the agent's list (or of every selected candidate) and the principles
        sc, K, r = ctx.scenes[a], ctx.scenes[a]["K"], got[a]
        sub = np.arange(SIZES[a % 4]) if lists[a] is None else lists[a]
        keep = np.nonzero((sc["flags"][sub] & NEED) == NEED)[0] if lists[a] is None else np.arange(len(sub))
        if len(sub) == 0 or len(keep) == 0:
            assert r["min_risk_index"] == -1, a
            continue
        if K == 0:      # no risk obstacle: rows without an item -- every risk 0.0, the arg-min the smallest candidate index
            assert all(np.all(r[q][keep] == 0.0) for q in ROWS) and r["ego_risk_max"].shape == (len(sub), 0), a
            assert r["min_risk_index"] == int(sub[keep].min()), a
            continue
        P = [sc["planes"][n][sub[keep]] for n in PLANES]
        want = rcr.calc_risk_detail(*P, sc["preds"], sc["typ"], sc["modes"], HARM, **ego_of(a))
        for q in COLS + ROWS:
            assert rel_err(r[q][keep], want[q]) < 1e-12, (a, q)
        assert r["min_risk_index"] == rr.min_risk_index(r["ego_risk"][keep], r["obst_risk"][keep], sub[keep]), a
        if costs[a] is None:
            continue
        if costs[a].responsibility_mode == _abi.FX_RISK_RESP_REACH_SET:
            wr = [rcr.responsibility_reach_set(P[0][c], P[1][c], ctx.inps[a].dt, sc["sets"], want["obst_risk_max"][c], sc["keys"])[0]
                  for c in range(len(keep))]
        else:
            wr = [rcr.responsibility_action_space(want["obst_risk_max"][c], sc["preds"], sc["x0"], sc["th0"]) for c in range(len(keep))]
        wc = rcr.costs(want, r["boundary_harm"][keep], WEIGHTS, wr)
        tol = dict(bayes=(2 * K + 1) * 1e-12, equality=(2 * K + 1) * 1e-12, maximin=10e-12, ego=(2 * K + 1) * 1e-12,
                   responsibility=(2 * K + 1) * 1e-12)
        tol["total"] = sum(w * tol[n] for w, n in zip(WEIGHTS, rcr.NAMES))
        for q, t in tol.items():
            assert rel_err(r[q][keep], wc[q]) < t, (a, q)
        assert r["min_cost_index"] == rcr.argmin_index(r["total"][keep], sub[keep]), a


# ------------------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refusals(ctx):
    """n_agents = A + 1 and an agent listed twice (behind position 63) are refused by the four batched entries with the messages
    they have, outputs untouched, nothing allocated; the passes answer as before"""
    from tests import test_predprob_batch_gpu as m18, test_resp_batch_gpu as m19, test_risk_batch_gpu as m20, test_risk_costs_batch_gpu as m21
    e, A, scenes = ctx.eng, ctx.A, ctx.scenes
    INV = _abi.FX_ERR_INVALID_ARGUMENT
    before_call = e.risk_batch([sc["params"] for sc in scenes])
    before = e.device_bytes
    many = list(range(A)) + [A - 1]
    twice = list(range(A - 1)) + [A - 2]
    none = [None] * (A + 1)
    for name, r, un in (("predprob", m18._raw(e, many, n=A + 1), m18._untouched), ("resp", m19._raw(e, many, scenes, n=A + 1), m19._untouched),
                        ("risk", m20._raw(e, many, scenes, none, n=A + 1), m20._untouched),
                        ("risk costs", m21._raw(e, many, scenes, none, n=A + 1), m21._untouched)):
        assert r[0] == INV and f"n_agents {A + 1}" in r[1] and un(r), (name, r[:2])
    for name, r, un in (("predprob", m18._raw(e, twice), m18._untouched), ("resp", m19._raw(e, twice, scenes), m19._untouched),
                        ("risk", m20._raw(e, twice, scenes, none[:A]), m20._untouched),
                        ("risk costs", m21._raw(e, twice, scenes, none[:A]), m21._untouched)):
        assert r[0] == INV and f"agent {A - 2} listed twice" in r[1] and un(r), (name, r[:2])
    assert e.device_bytes == before
    for a, r in enumerate(e.risk_batch([sc["params"] for sc in scenes])):
        _risk_same(r, before_call[a], ("after the refusals", a))
