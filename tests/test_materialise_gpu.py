"""Listed candidates of a select-only plan step, materialised beside it (fx_materialise_candidates_agent).

The list kernel is the generic evaluation kernel at one lane per candidate with its index read from a list: the same walk in a
third kernel.  So the requirement against the bundle the generic kernel stores (set_tuning(1, 0, 1)) is equality, bit for bit, of
every part -- planes, coefficients, horizon lengths, raw costs, costs, flag words, boundary steps -- and against the select-only
step it follows (automatic tuning: another kernel, whose cost sums associate differently) rtol = 1e-12 on the cost, the figure
test_hip_parity.test_generic_and_grid_kernels_agree_bitwise holds between kernels, and equal flag words."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, synthetic
from tests.test_hip_parity import CASES, compare, hip_hulls

pytestmark = pytest.mark.gpu

PARTS = ("lon", "lat", "tau_lat", "traj_len", "raw_costs", "cost", "flags")
BITWISE_KW = dict(ref_kind="scurve", kappa=0.02, v0=9.0, grid=(7, 9, 33), n_obstacles=6, draw_traj_set=True, kinematic_debug=True)
SMALL_KW = dict(ref_kind="arc", v0=10.0, grid=(5, 9, 11), n_obstacles=4)


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=120_000, max_steps=60, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64, max_agents=8)
    yield e
    e.close()


def id_lists(C_):
    """the lists of the issue: one, two out of order, two waves with the second ragged (70 + 5 duplicates, unsorted), exactly
    one wave, every candidate"""
    rng = np.random.default_rng(11)
    seventy = rng.choice(C_, size=min(70, C_), replace=False)
    ragged = np.concatenate([seventy, seventy[:5]])
    rng.shuffle(ragged)
    return [np.array([0]), np.array([C_ - 1, 0]), ragged, rng.choice(C_, size=min(64, C_), replace=False), np.arange(C_)]


def bundle_twin(eng, kw, tuning=(1, 0, 1)):
    """the inputs in bundle mode on the generic kernel: every part of every candidate, and the step's result"""
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    eng.set_tuning(*tuning)
    try:
        res = eng.plan_step(inp)
        rows = eng.candidates(np.arange(inp.n_candidates))
        cost, flags = eng.costs()
    finally:
        eng.set_tuning(0, 0, 0)
    assert np.array_equal(rows["cost"], cost) and np.array_equal(rows["flags"], flags)
    return inp, res, rows


def stored_mask(inp, flags):
    """candidates whose planes the bundle run defines: those test_hip_parity.compare holds to the oracle"""
    ret = (flags & _abi.FX_FLAG_RETURNED) != 0
    return ret & (((flags & _abi.FX_FLAG_COSTED) != 0) | bool(inp.draw_traj_set))


def assert_rows_equal(got, want, ids, inp, boundary=False):
    for k in PARTS:
        assert np.array_equal(got[k], want[k][ids]), k
    st = stored_mask(inp, want["flags"][ids])
    assert st.any() or len(ids) < 64
    assert np.array_equal(got["planes"][st], want["planes"][ids][st]), "planes"
    if boundary:
        assert np.array_equal(got["boundary_step"], want["boundary_step"][ids]), "boundary_step"
    else:
        assert got["boundary_step"] is None


def select_only(kw):
    return synthetic.make_inputs(hull_builder=hip_hulls(), write_bundle=False, write_costmap=False, **kw)


@pytest.mark.parametrize("stop", [None, 28.0])
def test_bit_identical_with_the_bundle_and_consistent_with_the_step(eng, stop):
    kw = dict(BITWISE_KW, stop_point_s=stop)
    inp_b, _, want = bundle_twin(eng, kw)
    inp = select_only(kw)
    eng.plan_step(inp)
    cost, flags = eng.costs()
    assert inp.n_candidates % 64 != 0 and inp.n_candidates > 2048   # (7 x 9 x (33 + d0): 34 waves, the last ragged)
    for ids in id_lists(inp.n_candidates):
        got = eng.materialise(ids)
        assert_rows_equal(got, want, ids, inp_b)
        # against the step it follows (another kernel): the cost to 1e-12, the flag words equal
        assert np.array_equal(got["flags"], flags[ids])
        assert np.allclose(got["cost"], cost[ids], rtol=1e-12, atol=0)
    with pytest.raises(Exception):
        eng.sample(0)   # the step's own outputs are what they were: no bundle


def test_the_step_is_untouched(eng):
    inp = select_only(BITWISE_KW)
    res = eng.plan_step(inp)
    before = (eng.costs(), eng.topk(32), eng.step_info())
    eng.materialise(id_lists(inp.n_candidates)[2])
    eng.materialise(np.arange(inp.n_candidates))
    after = (eng.costs(), eng.topk(32), eng.step_info())
    for a, b in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(a, b)
    assert before[2] == after[2]
    assert eng.finish()[0] == res   # the published result block: counters, histogram, winner


FORMS = {
    "matrix": dict(SMALL_KW, as_matrix=True),
    "low_velocity": dict(SMALL_KW, v0=1.5),
    "horizon5": dict(SMALL_KW, horizon=5.0, n_pred=50),
    "no_obstacles": dict(SMALL_KW, n_obstacles=0),
    "windowed_costs": dict(SMALL_KW, cost_weights=dict(synthetic.DEFAULT_COST_WEIGHTS, acceleration=0.3, distance_to_obstacles=0.7)),
    "road_boundary": dict(SMALL_KW, road_half_width=2.6),
}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_every_input_form(eng, name):
    kw = FORMS[name]
    inp_b, _, want = bundle_twin(eng, kw)
    inp = select_only(kw)
    assert inp.n_samples == (51 if name == "horizon5" else 31)
    eng.plan_step(inp)
    cost, flags = eng.costs()
    boundary = name == "road_boundary"
    if boundary:
        assert (want["boundary_step"] >= 0).any()
    for ids in id_lists(inp.n_candidates)[1:]:
        got = eng.materialise(ids)
        assert_rows_equal(got, want, ids, inp_b, boundary)
        assert np.array_equal(got["flags"], flags[ids]) and np.allclose(got["cost"], cost[ids], rtol=1e-12, atol=0)


def test_sharded_step_takes_local_ids(eng):
    inp_b = synthetic.make_inputs(hull_builder=hip_hulls(), **SMALL_KW)
    inp_b.shard = (37, 200)
    eng.set_tuning(1, 0, 1)
    try:
        eng.plan_step(inp_b)
        want = eng.candidates(np.arange(200))
    finally:
        eng.set_tuning(0, 0, 0)
    inp = select_only(SMALL_KW)
    inp.shard = (37, 200)
    eng.plan_step(inp)
    for ids in id_lists(200)[1:]:
        assert_rows_equal(eng.materialise(ids), want, ids, inp_b)
    with pytest.raises(ValueError):
        eng.materialise([200])
    pkg = eng.materialised_package(5)
    assert pkg.index == 37 + 5   # (the package speaks global indices, as fx_read_package does)


def test_two_agents_keep_their_sets_apart(eng):
    kws = [SMALL_KW, dict(ref_kind="scurve", kappa=0.02, v0=8.0, grid=(4, 7, 9), n_obstacles=3)]
    wants = []
    eng.set_tuning(1, 0, 1)
    try:
        inps_b = [synthetic.make_inputs(hull_builder=hip_hulls(), **kw) for kw in kws]
        eng.plan_batch(inps_b)
        wants = [eng.candidates(np.arange(i.n_candidates), agent=a) for a, i in enumerate(inps_b)]
    finally:
        eng.set_tuning(0, 0, 0)
    eng.plan_batch([select_only(kw) for kw in kws])
    ids0, ids1 = np.array([3, 400, 17]), np.array([250, 3, 9, 9])
    got0 = eng.materialise(ids0, agent=0)
    got1 = eng.materialise(ids1, agent=1)
    assert_rows_equal(got0, wants[0], ids0, inps_b[0])
    assert_rows_equal(got1, wants[1], ids1, inps_b[1])
    # agent 0's set is still there, and it is agent 0's: 400 is no candidate of agent 1, 250 is not in agent 0's set
    again = _read(eng, 0, ids0, inps_b[0])
    assert np.array_equal(again["planes"], got0["planes"]) and np.array_equal(again["cost"], got0["cost"])
    with pytest.raises(ValueError):
        _read(eng, 0, np.array([250]), inps_b[0])


def _read(eng, agent, ids, inp):
    """fx_read_materialised_agent alone (no new set)"""
    from frenetix_motion_planner_amd._lib import check, lib
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n = len(ids)
    planes, cost = np.empty((n, _abi.FX_NUM_PLANES, inp.n_samples)), np.empty(n)
    check(lib().fx_read_materialised_agent(eng._ctx, agent, n, ids.ctypes.data, planes.ctypes.data, None, None, None, cost.ctypes.data,
                                           None, None))
    return dict(planes=planes, cost=cost)


class _RowsAsEngine:
    """the materialised rows of EVERY candidate behind the read-back calls test_hip_parity.compare makes"""

    def __init__(self, rows):
        self.r = rows

    def costs(self, agent=0):
        return self.r["cost"], self.r["flags"]

    def costmap(self, agent=0):
        return self.r["raw_costs"]

    def bundle(self, agent=0):
        return self.r["planes"]

    def coeffs(self, g, agent=0):
        return self.r["lon"][g], self.r["lat"][g], int(self.r["traj_len"][g]), float(self.r["tau_lat"][g])

    def sample(self, g, agent=0):
        return self.r["planes"][g]


def test_materialised_rows_against_the_oracle(eng):
    from oracle import oracle
    kw = CASES["dense_prod_obs"]
    ref_inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
    out = oracle.plan_step(ref_inp)
    res = eng.plan_step(select_only(kw))
    rows = eng.materialise(np.arange(ref_inp.n_candidates))
    # compare() reads its tolerances' switches from the inputs: those of the bundle-mode case, whose parts the rows all have
    compare(_RowsAsEngine(rows), synthetic.make_inputs(hull_builder=hip_hulls(), **kw), out, res, ref_inp=ref_inp)


def test_errors_leave_the_previous_set_readable():
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = select_only(SMALL_KW)
    C_ = inp.n_candidates
    with FrenetEngine(max_candidates=C_) as e:
        L = lib()
        one = np.array([1], np.int64)
        assert L.fx_materialise_candidates_agent(e._ctx, 0, 1, one.ctypes.data) == _abi.FX_ERR_NOT_READY   # before any step
        e.plan_step(inp)
        ids = np.array([7, 3, 450], np.int64)
        first = e.materialise(ids)
        with pytest.raises(ValueError):
            e.materialise([C_])
        bad = np.array([3, C_], np.int64)
        assert L.fx_materialise_candidates_agent(e._ctx, 0, 2, bad.ctypes.data) == _abi.FX_ERR_INVALID_ARGUMENT
        assert L.fx_materialise_candidates_agent(e._ctx, 0, -1, one.ctypes.data) == _abi.FX_ERR_INVALID_ARGUMENT
        assert L.fx_materialise_candidates_agent(e._ctx, 0, 2, None) == _abi.FX_ERR_INVALID_ARGUMENT
        again = _read(e, 0, ids, inp)
        assert np.array_equal(again["planes"], first["planes"]) and np.array_equal(again["cost"], first["cost"])
        # an id outside the set
        with pytest.raises(ValueError, match="status -2"):
            _read(e, 0, np.array([8]), inp)
        # the inputs rewritten without an evaluation: the re-walk would use another state, and the set is over
        e.update_state(e._state_update_of(inp))
        assert L.fx_materialise_candidates_agent(e._ctx, 0, 1, one.ctypes.data) == _abi.FX_ERR_NOT_READY
        with pytest.raises(ValueError, match="status -2"):
            _read(e, 0, ids, inp)
        e.evaluate()
        e.finish()
        with pytest.raises(ValueError, match="status -2"):
            _read(e, 0, ids, inp)   # a new step: a new set is needed
        assert np.array_equal(e.materialise(ids)["planes"], first["planes"])
        assert L.fx_materialise_candidates_agent(e._ctx, 0, 0, None) == _abi.FX_OK   # n == 0 clears
        with pytest.raises(ValueError, match="status -2"):
            _read(e, 0, ids, inp)


def test_device_bytes_unchanged_until_the_first_call():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = select_only(SMALL_KW)
    with FrenetEngine(max_candidates=inp.n_candidates) as a, FrenetEngine(max_candidates=inp.n_candidates) as b:
        a.plan_step(inp)
        b.plan_step(inp)
        assert a.device_bytes == b.device_bytes
        b.materialise([1, 2, 3])
        grown = b.device_bytes
        assert grown > a.device_bytes
        b.materialise([5])
        assert b.device_bytes == grown   # grow-only: a shorter list reuses the block


def test_risk_on_a_step_without_a_bundle():
    """test_risk_gpu.py's setting run select-only: risk(), risk_detail() and risk_costs() of 100 materialised candidates equal the
    same calls on the bundle-mode twin (generic kernel), arg-min indices included"""
    from frenetix_motion_planner_amd import risk
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from tests.test_risk_gpu import BASE, EGO, HARM, _predictions
    kw = dict(ref_kind="arc", v0=10.0, grid=(8, 16, 16), n_obstacles=4)
    inp_b = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    inp = select_only(kw)
    weights = [1.0, 0.5, 2.0, 0.25, 1.5]
    with FrenetEngine(max_candidates=inp.n_candidates) as e:
        e.set_tuning(1, 0, 1)
        e.plan_step(inp_b)
        _, flags = e.costs()
        planes = {n: e.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(7))
        tabs = risk.obstacle_tables(preds, typ)
        e.set_risk_obstacles(tabs)
        params = risk.risk_params(BASE, HARM, **EGO)
        ok = np.nonzero((flags & 0xB) == 0xB)[0]
        _, _, best = e.risk(params, ok)
        rng = np.random.default_rng(3)
        ids = np.unique(np.concatenate([rng.choice(ok, size=99, replace=False), [best]]))[::-1].copy()   # unsorted on purpose
        ids = ids[:100]
        assert best in ids
        bh = rng.random(len(ids))
        cp = lambda: risk.risk_cost_params(weights, boundary_harm=bh)
        want = (e.risk(params, ids), e.risk_detail(params, ids), e.risk_costs(params, cp(), ids))
        assert want[0][2] == best
        e.set_tuning(0, 0, 0)
        e.plan_step(inp)
        e.set_risk_obstacles(tabs)
        with pytest.raises(ValueError, match="status -2"):
            e.risk(params, ids)   # nothing materialised yet
        e.materialise(ids)
        got = (e.risk(params, ids), e.risk_detail(params, ids), e.risk_costs(params, cp(), ids))
        assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1]) and got[0][2] == want[0][2]
        for g, w in zip(got[1:], want[1:]):
            assert g.keys() == w.keys()
            for k in w:
                assert np.array_equal(g[k], w[k]), k
        with pytest.raises(ValueError, match="status -2"):
            e.risk(params)   # ids = None still needs the whole bundle
        outside = np.setdiff1d(ok, ids)[:1]
        with pytest.raises(ValueError, match="status -2"):
            e.risk(params, np.concatenate([ids[:3], outside]))
        with pytest.raises(ValueError, match="status -2"):
            e.risk_costs(params, risk.risk_cost_params(weights), None)


def test_materialised_package_equals_the_winner_package(eng):
    inp_b = synthetic.make_inputs(hull_builder=hip_hulls(), **SMALL_KW)
    eng.set_package(True)
    eng.set_tuning(1, 0, 1)
    try:
        res = eng.plan_step(inp_b)
        want = eng.package(0, 0.125)
    finally:
        eng.set_tuning(0, 0, 0)
        eng.set_package(False)
    assert want is not None
    res2 = eng.plan_step(select_only(SMALL_KW))
    assert res2["best_index"] == res["best_index"]
    eng.materialise([res2["best_index"], 0])
    got = eng.materialised_package(res2["best_index"], 0.125)
    for f, _ in _abi.FxPackage._fields_:
        a, b = getattr(got._pkg, f), getattr(want._pkg, f)
        assert (list(a) == list(b)) if hasattr(a, "__len__") else a == b, f
    assert np.array_equal(got.block, want.block)


SAMPLE_VIEWS = (lambda t: t.cartesian.x, lambda t: t.cartesian.kappa, lambda t: t.curvilinear.d, lambda t: t.costMap,
                lambda t: t.feasabilityMap, lambda t: t.sampling_parameters, lambda t: t.actual_traj_length, lambda t: t.cost)


def _same(a, b):
    return a == b if isinstance(a, (dict, int, float)) else np.array_equal(a, b)


def test_samples_of_a_select_only_step_before_and_after_the_next_step(eng):
    from frenetix_motion_planner_amd.trajectories import PlanStepResult
    kw = dict(SMALL_KW, draw_traj_set=True, kinematic_debug=True)
    inp_b = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    ids = [int(g) for g in id_lists(inp_b.n_candidates)[2][:12]]
    eng.set_tuning(1, 0, 1)
    try:
        twin = PlanStepResult(eng, inp_b, eng.plan_step(inp_b))
        want = {g: [view(twin.sample(g)) for view in SAMPLE_VIEWS] for g in ids}
    finally:
        eng.set_tuning(0, 0, 0)
    inp = select_only(kw)
    step = PlanStepResult(eng, inp, eng.plan_step(inp))
    unlisted = next(g for g in range(inp.n_candidates) if g not in ids)
    step.materialise(ids[6:] + ids[:6])
    kept = [step.sample(g) for g in ids]
    other = step.sample(unlisted)
    for t in kept[:6]:   # read before the next step ...
        assert all(_same(view(t), w) for view, w in zip(SAMPLE_VIEWS, want[t.uniqueId]))
    with pytest.raises(ValueError, match="status -2"):
        other.cartesian
    eng.plan_step(select_only(dict(kw, v0=7.0)))
    for t in kept:       # ... and after it, the second half for the first time
        assert all(_same(view(t), w) for view, w in zip(SAMPLE_VIEWS, want[t.uniqueId])), t.uniqueId
    with pytest.raises((ValueError, RuntimeError)):
        other.cartesian


def _pair_columns(pair):
    cart, cl, lon, lat = pair
    cols = [[getattr(s, f) for s in cart] for f in ("orientation", "velocity", "acceleration", "yaw_rate", "steering_angle")]
    cols += [[s.position[0] for s in cart], [s.position[1] for s in cart]]
    cols += [[c[f] for c in cl] for f in ("velocity", "acceleration", "orientation", "yaw_rate")]
    cols += [[c["position"][0] for c in cl], [c["position"][1] for c in cl]]
    return [np.asarray(c, float) for c in cols] + [np.asarray(list(lon), float), np.asarray(list(lat), float)]


def test_planner_on_a_sparse_set_plans_what_the_bundle_planner_plans():
    from tests.test_hip_planner import make_planner
    a, _ = make_planner()
    b, _ = make_planner(sparse_bundle_k=32)
    try:
        pa, pb = a.plan(), b.plan()
        assert pa is not None and pb is not None
        assert not b.last_step.inputs.write_bundle and a.last_step.inputs.write_bundle
        assert b.optimal_trajectory.uniqueId == a.optimal_trajectory.uniqueId
        assert b.last_step.result["best_index"] == a.last_step.result["best_index"]
        assert b.last_step.result["reason_hist"] == a.last_step.result["reason_hist"]
        for ca, cb in zip(_pair_columns(pa), _pair_columns(pb)):
            assert np.allclose(cb, ca, rtol=1e-12, atol=0)
        assert set(b.optimal_trajectory.costMap) == set(a.optimal_trajectory.costMap)
        # a second step: the set of the first is gone with it, the second step's is made afresh
        pa2, pb2 = a.plan(), b.plan()
        assert b.optimal_trajectory.uniqueId == a.optimal_trajectory.uniqueId
        for ca, cb in zip(_pair_columns(pa2), _pair_columns(pb2)):
            assert np.allclose(cb, ca, rtol=1e-12, atol=0)
        # the k = 0 planner's context owns what it always did: the sparse block exists only where it was asked for
        assert a.engine.device_bytes < b.engine.device_bytes
    finally:
        a.close()
        b.close()


def test_blocked_planner_min_risk_fallback_on_a_sparse_set():
    from tests.test_risk_planner import _with_model
    chosen = []
    for k in (0, 32):
        rp = _with_model(sampling_min=1, sampling_max=3, sparse_bundle_k=k)
        rp.set_fallback_selector("min_risk")
        try:
            pair = rp.plan()
            step = rp.last_step
            assert pair is not None and step.result["best_index"] == -1 and step.result["n_feasible"] > 0
            best = rp.optimal_trajectory
            chosen.append((best.uniqueId, step.result["reason_hist"], best._ego_risk, best._obst_risk, _pair_columns(pair)))
        finally:
            rp.close()
    assert chosen[0][:2] == chosen[1][:2]
    assert chosen[0][2] == chosen[1][2] and chosen[0][3] == chosen[1][3]
    for ca, cb in zip(chosen[0][4], chosen[1][4]):
        assert np.allclose(cb, ca, rtol=1e-12, atol=0)
