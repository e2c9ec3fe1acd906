"""The items of the trajectory-risk walk (fx_risk_kernel.h): the chunk size changes no bit.  Every output of
risk(), risk_detail() and risk_costs() with the automatic chunk size, with one step per chunk and with seven is the one with ONE
chunk per obstacle -- the serial step order -- on the same context, step and obstacles, bit for bit (np.array_equal, NaN rows
equal); so are the batches of the partials, an agent of a batch context and calls that share the block.

These tests once held the item kernels to a second walk, one lane per candidate, which alone was held to the references; that walk
is gone.  The item kernels are now held directly, at 1e-12, to the NumPy restatements and to the reference's own values by
tests/test_risk_gpu.py, test_risk_costs_gpu.py and test_risk_golden.py, which run unedited on them.

Why equality and not a tolerance: every per-step value comes from the same device function on the same operands, and what is kept
of them is a maximum (fmax from -inf: associative and commutative bit for bit) or the first maximum of a list (strict >, chunks
combined in chunk order).  The chunk size decides how many waves a call has and nothing else."""
import numpy as np
import pytest

from tests.test_risk_costs_gpu import COLS, WEIGHTS, _reach_sets, _same
from tests.test_risk_gpu import BASE, EGO, HARM

pytestmark = pytest.mark.gpu

GRID = (8, 16, 16)
NEED = 0xB   # VALID | FEASIBLE | RETURNED
MODES = {"log_reg": BASE, "mahalanobis": dict(BASE, fast_prob_mahalanobis=True), "ref_speed": dict(BASE, harm_mode="ref_speed", ignore_angle=True)}
COUNTS = (1, 63, 64, 65, 130, None)


def _make(**kw):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    args = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=GRID, n_obstacles=4)
    args.update(kw)
    return synthetic.make_inputs(**args)


def _planes(eng, agent=0):
    return {n: eng.plane(n, agent).T.copy() for n in ("x", "y", "theta", "v")}   # [C, S]


@pytest.fixture(scope="module")
def step():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = _make()
    eng = FrenetEngine(max_candidates=inp.n_candidates, device=0)
    eng.plan_step(inp)
    _, flags = eng.costs()
    yield eng, inp, flags, _planes(eng)
    eng.close()


def _obstacles(planes, ok, K):
    """Up to four obstacles that drive beside candidates, 6.5 m to their left or right: outside the 5 m gate of every candidate at
    the common start, later inside it for the candidates that swerve towards them and never for the ones that swerve away -- lanes
    of one tile differ.  A protected one and an unprotected one over the whole horizon, a protected one whose prediction ends seven
    steps early (pl ends inside a chunk of 7 and of the automatic size), and one with a single position (npos = 1: one harm, no
    valid probability record)."""
    S = planes["x"].shape[1]
    rng = np.random.default_rng(3)
    spec = [("car", S - 1, 0.0, 6.5), ("pedestrian", S - 1, 0.8, -6.5), ("truck", S - 7, -0.95, 6.5), ("bicycle", 1, 0.2, -6.5)][:K]
    preds, typ = {}, {}
    for k, (kind, P, rho, side) in enumerate(spec):
        c = ok[(7 + 37 * k) % len(ok)]
        th = planes["theta"][c, :P]
        off = rng.normal(0, 0.2, 2)
        sx, sy = 0.4 + 0.1 * k, 0.5
        cov = np.tile(np.array([[sx * sx, rho * sx * sy], [rho * sx * sy, sy * sy]]), (P, 1, 1)) * np.linspace(1, 3, P)[:, None, None]
        pos = np.stack([planes["x"][c, :P] - side * np.sin(th) + off[0], planes["y"][c, :P] + side * np.cos(th) + off[1]], axis=1)
        preds[200 + k] = dict(pos_list=pos, cov_list=cov, orientation_list=th + rng.normal(0, 0.2),
                              v_list=np.abs(planes["v"][c, :P] + rng.normal(0, 2)), shape=dict(length=4.0 + 0.3 * k, width=1.8))
        typ[200 + k] = kind
    return preds, typ


def _calls(eng, params, cost, lists):
    """risk, risk_detail and risk_costs (action-space and, where given, reach-set responsibility) for every id list"""
    from frenetix_motion_planner_amd import risk
    out = {}
    for name, ids in lists.items():
        out[name, "risk"] = eng.risk(params, ids)
        out[name, "detail"] = eng.risk_detail(params, ids)
        for mode, resp in cost.items():
            out[name, mode] = eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, responsibility=resp), ids)
    return out


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K", [0, 1, 3, 4])
def test_chunk_size_changes_no_bit(step, K, mode):
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd._lib import lib
    eng, inp, flags, planes = step
    S, C = inp.n_samples, inp.n_candidates
    assert S == 31 and (S - 1) % 7 != 0
    modes = MODES[mode]
    ok = np.nonzero((flags & NEED) == NEED)[0]
    assert 130 < len(ok) < C
    preds, typ = _obstacles(planes, ok, K)
    tabs = risk.obstacle_tables(preds, typ, mahalanobis=modes["fast_prob_mahalanobis"])
    if K >= 3:
        assert set(tabs["cls"][:3]) == {0, 1} and list(tabs["n_pos"][:3]) == [S - 1, S - 1, S - 7]
    if K == 4:
        assert tabs["n_pos"][3] == 1
    eng.set_risk_obstacles(tabs)
    keys = list(preds)
    cost = {"action": risk.action_space_responsibility(preds, np.array([planes["x"][ok[0], 0], planes["y"][ok[0], 0]]),
                                                       float(planes["theta"][ok[0], 0]) + 0.5)}
    if K:
        eng.set_reach_sets(risk.reach_set_tables(_reach_sets(planes, keys, ok[::3], inp.dt), keys, inp.dt, S))
        cost["reach"] = "reach_set"
    params = risk.risk_params(modes, HARM, **EGO)
    # (lists spread over the whole grid: the 64 lanes of a tile hold candidates of every end time, velocity and offset)
    lists = {n: (None if n is None else ok[np.linspace(0, len(ok) - 1, n).astype(int)]) for n in COUNTS}
    try:
        lib().fx_risk_items_set_chunk_steps(S - 1)   # one chunk per obstacle: its steps in their serial order
        assert lib().fx_risk_items_chunk_steps(C, S, max(K, 1)) == S - 1
        want = _calls(eng, params, cost, lists)
        if K and mode != "mahalanobis":
            # the gate diverges inside a tile: of the first 64 listed candidates some come within 5 m of obstacle 0 and some never do
            r0 = want[64, "detail"]["obst_risk_max"][:, 0]
            assert (r0 > 0).any() and (r0 == 0).any()
            assert (want[None, "detail"]["obst_risk_max"][ok][:, :3] > 0).any(axis=0).all()   # (every obstacle with a record is met by somebody)
        if K >= 3:
            assert np.nanmax(want[None, "detail"]["obst_harm_occ"]) > 0   # (a maximum above 0.001 somewhere: not a comparison of zeros)
        lib().fx_risk_items_set_chunk_steps(0)   # the automatic size
        got = _calls(eng, params, cost, lists)
        for key, w in want.items():
            assert _same(got[key], w), key
        assert eng.last_risk_ms > 0
        some = {n: lists[n] for n in (65, None)}
        for cs in (1, 7):
            lib().fx_risk_items_set_chunk_steps(cs)
            assert lib().fx_risk_items_chunk_steps(C, S, max(K, 1)) == cs
            got = _calls(eng, params, cost, some)
            for key, g in got.items():
                assert _same(g, want[key]), (cs, key)
    finally:
        lib().fx_risk_items_set_chunk_steps(0)
    full = want[None, "detail"]
    off = np.setdiff1d(np.arange(C), ok)
    assert all(np.all(np.isnan(full[q][off])) for q in COLS + ("ego_risk", "obst_harm_occ"))


def test_first_maximum_across_chunks():
    """The ego stands still in front of a stop point at its own position, so the grid holds candidates that never move: (x, y,
    theta) bit-constant over the horizon.  A stationary obstacle beside them with a constant covariance and orientation and a
    v_list that grows per step: the probability of every step is computed from the same operands -- the same number, in every
    chunk of 1 and of 7 steps -- the harm is not, and obst_harm_occ must be the harm of the FIRST step, in whatever chunk the
    later, equal maxima lie."""
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from tests import risk_costs_restatement as rcr
    inp = _make(v0=0.0, v_des=0.0, n_obstacles=0, stop_point_s=0.0)
    S = inp.n_samples
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        planes = _planes(eng)
        still = np.nonzero((np.ptp(planes["x"], axis=1) == 0) & (np.ptp(planes["y"], axis=1) == 0) & (np.ptp(planes["theta"], axis=1) == 0))[0]
        assert len(still) > 0, "no candidate with bit-constant (x, y) and theta"
        c = still[0]
        th = float(planes["theta"][c, 0])
        P = S - 1
        pos = np.array([planes["x"][c, 0] + 2.0 * np.cos(th) - 0.5 * np.sin(th), planes["y"][c, 0] + 2.0 * np.sin(th) + 0.5 * np.cos(th)])
        preds = {7: dict(pos_list=np.tile(pos, (P, 1)), cov_list=np.tile(np.array([[0.5, 0.1], [0.1, 0.4]]), (P, 1, 1)),
                         orientation_list=np.full(P, th + 0.3), v_list=np.linspace(1.0, 15.0, P), shape=dict(length=4.5, width=1.8))}
        typ = {7: "car"}
        eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
        params = risk.risk_params(BASE, HARM, **EGO)
        ids = np.concatenate([still[:3], np.arange(0, inp.n_candidates, 29)])
        try:
            lib().fx_risk_items_set_chunk_steps(S - 1)   # one chunk: the steps in their serial order
            walk = eng.risk_detail(params, ids)
        finally:
            lib().fx_risk_items_set_chunk_steps(0)
        sub = ids[:1]
        ref = rcr.calc_risk_detail(*[planes[n][sub] for n in ("x", "y", "theta", "v")], preds, typ, BASE, HARM, **EGO)
        # the precondition: a probability above the 0.001 of the rule, the first step's harm well below the horizon's largest
        assert walk["obst_harm_occ"][0] > 0 and walk["obst_harm_max"][0, 0] > walk["obst_harm_occ"][0] + 1e-3
        assert abs(walk["obst_harm_occ"][0] - ref["obst_harm_occ"][0]) < 1e-12
        # ... and the tie itself: the restated per-step probabilities of this candidate, from the read-back planes and the
        # prediction as it was handed over, reach their maximum at the first step and again, bit for bit, in other chunks
        prob = rcr.probability(*[planes[n][sub] for n in ("x", "y", "theta")], preds[7], BASE, EGO["ego_length"], EGO["ego_width"])[0]
        assert prob.shape == (S - 1,) and prob[0] == prob.max() > 0.001
        for cs in (1, 7):
            tied = [a // cs for a in range(0, S - 1, cs) if prob[a:a + cs].max() == prob.max()]
            assert len(tied) >= 2 and tied[0] == 0, (cs, prob)
        harm = rcr._harm(*[planes[n][sub] for n in ("x", "y", "theta", "v")], preds[7], "car", BASE, HARM, EGO["ego_mass"])[1][0]
        assert np.all(harm[1:] > harm[0])   # (any later tied step would give a larger harm: `>=` in a combine would show)
        try:
            for cs in (0, 1, 7):   # (1 and 7: the tied maximum lies in every chunk)
                lib().fx_risk_items_set_chunk_steps(cs)
                assert _same(eng.risk_detail(params, ids), walk), cs
        finally:
            lib().fx_risk_items_set_chunk_steps(0)


def _rows(res, rows):
    """the per-candidate rows of a risk_detail result"""
    return {k: v[rows] for k, v in res.items() if isinstance(v, np.ndarray)}


def test_more_than_one_batch_of_partials(step):
    """The partials of one batch stay within 64 MiB: with K = 20 obstacles and one step per chunk a candidate's share of the detail
    pass is 7 values x 20 obstacles x 30 chunks x 8 bytes = 33 600 bytes, a batch holds 1 984 candidates (31 whole tiles) and the
    2 176 candidates of the grid take two -- the second one ragged, 192 candidates in 3 tiles.  The base: the second batch's
    candidates as a list of their own, which one batch holds."""
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd._lib import lib
    from tests.test_risk_gpu import _predictions
    eng, inp, flags, planes = step
    S, C = inp.n_samples, inp.n_candidates
    assert (64 << 20) // (7 * 20 * (S - 1) * 8) // 64 * 64 == 1984 < C
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=20)
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
    params = risk.risk_params(BASE, HARM, **EGO)
    ok = np.nonzero((flags & NEED) == NEED)[0]
    assert ok.max() >= 1984   # (selected candidates in the second batch)
    second = np.arange(1984, C)
    sel = ok[ok >= 1984]
    assert len(second) <= 1984
    want = _rows(eng.risk_detail(params, second), slice(None))
    assert (want["obst_risk_max"][sel - 1984] > 0).any()
    try:
        lib().fx_risk_items_set_chunk_steps(1)
        full, rev = eng.risk_detail(params), eng.risk_detail(params, np.arange(C)[::-1])
    finally:
        lib().fx_risk_items_set_chunk_steps(0)
    assert _same(_rows(rev, C - 1 - second), want)                       # a listed candidate is evaluated whatever its flags say
    assert _same(_rows(full, sel), _rows(want, sel - 1984))              # every candidate: the selected ones ...
    off = np.setdiff1d(second, sel)
    assert all(np.all(np.isnan(v)) for v in _rows(full, off).values())   # ... and NaN rows for the others


def test_agent_of_a_batch_context():
    """Agent 1 of a batch context returns what the same agent returns planned alone on a fresh engine"""
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inps = [_make(grid=(3, 5, 5)), _make(grid=(6, 7, 9), v0=8.0)]
    params = risk.risk_params(BASE, HARM, **EGO)
    cost = lambda: risk.risk_cost_params(WEIGHTS, responsibility=np.array([1.0, 0.0, 1.0]))
    with FrenetEngine(max_candidates=max(i.n_candidates for i in inps), device=0, max_agents=2) as eng:
        eng.plan_batch(inps)
        _, flags = eng.costs(1)
        planes = _planes(eng, 1)
        ok = np.nonzero((flags & NEED) == NEED)[0]
        assert len(ok) > 64
        preds, typ = _obstacles(planes, ok, 3)
        tabs = risk.obstacle_tables(preds, typ)
        eng.set_risk_obstacles(tabs, agent=1)
        got = [eng.risk(params, agent=1), eng.risk_detail(params, ok[:70], agent=1), eng.risk_costs(params, cost(), agent=1)]
    assert np.nanmax(got[2]["obst_harm_occ"]) > 0
    assert np.nanmax(got[1]["obst_risk_max"]) > 0
    with FrenetEngine(max_candidates=inps[1].n_candidates, device=0) as alone:
        alone.plan_step(inps[1])
        assert _same(alone.costs()[1], flags) and _same(_planes(alone), planes)   # (the same step: what the passes read)
        alone.set_risk_obstacles(tabs)
        want = [alone.risk(params), alone.risk_detail(params, ok[:70]), alone.risk_costs(params, cost())]
    assert all(_same(g, w) for g, w in zip(got, want))


def test_items_share_the_block():
    """The partials live in the risk passes' grow-only block: the first, largest call grows it, a repetition and smaller calls do
    not, and the largest call returns, first and after the others, what it returns on a fresh engine (test_calls_share_one_block's
    property)."""
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = _make(grid=(6, 7, 3), n_obstacles=2)
    params = risk.risk_params(BASE, HARM, **EGO)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        _, flags = eng.costs()
        planes = _planes(eng)
        ok = np.nonzero((flags & NEED) == NEED)[0]
        preds, typ = _obstacles(planes, ok, 3)
        tabs = risk.obstacle_tables(preds, typ)
        cost = lambda: risk.risk_cost_params(WEIGHTS, responsibility=np.array([0.0, 1.0, 1.0]))
        calls = [lambda e: e.risk_costs(params, cost()), lambda e: e.risk(params, ok[::3]), lambda e: e.risk_detail(params, ok)]
        eng.set_risk_obstacles(tabs)
        b0 = eng.device_bytes
        first = calls[0](eng)
        b2 = eng.device_bytes
        assert b2 > b0
        items = [first] + [call(eng) for call in calls[1:]] + [calls[0](eng)]
        assert eng.device_bytes == b2
    assert _same(items[-1], first)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as fresh:   # only the first call, on a fresh engine
        fresh.plan_step(inp)
        fresh.set_risk_obstacles(tabs)
        assert fresh.device_bytes == b0
        assert _same(calls[0](fresh), first)
