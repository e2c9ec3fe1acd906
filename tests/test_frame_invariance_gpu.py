"""The plan step away from the world origin, on the device (frames and scenes: tests/frames.py; the oracle's side of the matter:
tests/test_frame_invariance_cpu.py; DESIGN.md section 2 "Away from the origin").

What exists only for scenes far from (0, 0) -- and which test here exercises it:
  * the hot table's origin (hot_origin_of, pack_obstacle_tables' ox / oy, K.ox / K.oy in the walk, the obstacle, grid, generic
    and list kernels): a. on every decomposition (prediction-cost column of the cost map at 1e-8, total cost at 1e-9, collision
    bits exactly), d. with a different origin per agent of one launch, e. in the list kernel behind materialise;
  * hot_gap_margin ("within ~1 km of the origin"): the collision bits of a. and b. at 5e6 m;
  * the second computation of the origin in fx_update_state: c.;
  * the single-precision wave-level cull: the collision bits and the prediction cost of a. on the obstacle kernel and the
    fused stage, b. across frames;
  * absolute coordinates in the road-boundary pieces and bins, the lanelet boxes and rays, the risk records: a. (boundary bit
    and boundary_step, lane_center_offset column), e. (risk, risk_costs), the inverse map and the bins on the CPU.

Which of these a wrong origin actually trips was tried with experiment builds of the library (not part of the repository):
  * hot_origin_of answering (0, 0), or reading the knot's (s, theta) fields instead of (x, y): the fx_obstacle_kernel legs of a.
    at UTM and UTM2 fail on the total cost (2.0e-9 and 8.6e-8 relative against the bound of 1e-9), and so do the obstacle-kernel
    legs of c. and d.  At KM, and on the fused stage and the generic kernel in every frame, the answers stay within the
    tolerances: those legs show that the decisions hold, not that the origin is set.
  * fx_update_state keeping the upload's origin: only the obstacle-kernel leg of c. fails (bit-identity with a fresh upload).
  * hot_gap_margin answering 0: nothing fails -- with a right origin the expanded circle form is evaluated on metres, and its
    rounding (1e-13) decides no pair of these scenes.  The margin is run at 5e6 m, not shown to be needed.
"""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import frames
from tests.frames import FAR, FRAMES, SCENES
from tests.test_hip_parity import COST_RTOL, FRAGILE, RESULT_KEYS, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=24_000, max_steps=40, max_ref_knots=512, max_obstacles=128, max_pred_steps=64, max_agents=4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    """a second context: fresh uploads beside the first one's resident, updated state"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=8192, max_steps=40, max_ref_knots=512, max_obstacles=32, max_pred_steps=64)
    yield e
    e.close()


def _automatic(e):
    e.set_tuning(0, 0, 0, 0, 0)
    e.set_obstacle_stage(0)


def _top(out):
    return float(np.abs(out["planes"][:, :2]).max())


def _xy_tol(f, out):
    """KM: compare() as every other test calls it.  UTM frames: the absolute (x, y) bound built from the oracle's own error."""
    return None if f in ("NEAR", "KM") else frames.xy_tol(f, _top(out))


# ------------------------------------------------------------------------------------------------- a. same frame, device vs oracle
def _grid_fused(e, mp):
    e.set_tuning(0, 0, 2)
    e.set_obstacle_stage(1)


def _obstacle_kernel(steps, wg):
    def force(e, mp):
        mp.setenv("FX_OBST_WG", wg)
        e.set_obstacle_stage(2, steps)
    return force


def _generic(lanes):
    def force(e, mp):
        e.set_tuning(lanes, 0, 1)
    return force


DECOMPOSITIONS = {
    "grid_fused": (_grid_fused, lambda i: i["grid_kernel"] == 1 and i["obstacle_kernel"] == 0),
    "obstacle_kernel_2_items": (_obstacle_kernel(2, "0"), lambda i: i["obstacle_kernel"] == 1 and i["obstacle_steps_per_item"] == 2 and i["obstacle_workgroup_waves"] == 0),
    "obstacle_kernel_2_workgroups": (_obstacle_kernel(2, "1"), lambda i: i["obstacle_kernel"] == 1 and i["obstacle_steps_per_item"] == 2 and i["obstacle_workgroup_waves"] == 15),
    "obstacle_kernel_5_items": (_obstacle_kernel(5, "0"), lambda i: i["obstacle_kernel"] == 1 and i["obstacle_steps_per_item"] == 5 and i["obstacle_workgroup_waves"] == 0),
    "obstacle_kernel_5_workgroups": (_obstacle_kernel(5, "1"), lambda i: i["obstacle_kernel"] == 1 and i["obstacle_steps_per_item"] == 5 and i["obstacle_workgroup_waves"] == 6),
    "generic_1_lane": (_generic(1), lambda i: i["grid_kernel"] == 0 and i["lanes_per_candidate"] == 1),
    "generic_8_lanes": (_generic(8), lambda i: i["grid_kernel"] == 0 and i["lanes_per_candidate"] == 8),
    "select_only": (lambda e, mp: None, lambda i: True),
}


@pytest.mark.parametrize("how", sorted(DECOMPOSITIONS))
@pytest.mark.parametrize("scene", ["arc_boundary", "scurve_boundary"])
@pytest.mark.parametrize("f", FAR)
def test_device_against_oracle_on_every_decomposition(eng, monkeypatch, f, scene, how):
    """(fx_obstacle_kernel is declined behind a walk with the road-boundary stage: those four legs run the scene without its
    boundary -- the same obstacles, candidates and collisions)"""
    if how.startswith("obstacle_kernel"):
        scene += "_open"
    ref_inp, out = frames.oracle_step(scene, f)
    more = dict(write_bundle=False, write_costmap=False) if how == "select_only" else {}
    inp = frames.hip_inputs(frames.scene_kw(scene), FRAMES[f], **more)
    force, ran_as_asked = DECOMPOSITIONS[how]
    try:
        force(eng, monkeypatch)
        res = eng.plan_step(inp)
        info = eng.step_info()
        assert ran_as_asked(info), info
        compare(eng, inp, out, res, ref_inp=ref_inp, xy_tol=_xy_tol(f, out))
        if inp.mode & _abi.FX_MODE_ROAD_BOUNDARY:
            walked = out["selectable"] & (out["margin"] >= FRAGILE)
            assert (out["boundary_step"][walked] >= 0).sum() > 50
            assert np.array_equal(eng.boundary_steps()[walked], out["boundary_step"][walked])
        assert res["best_index"] == out["result"]["best_index"] >= 0   # (no fragile candidate near the front of these scenes' cost order)
    finally:
        _automatic(eng)


@pytest.mark.parametrize("scene,tuning", [("arc_70_obstacles", (0, 0, 1)), ("lanelets", (0, 0, 0)), ("level2_jitter_debug", (0, 0, 0))])
@pytest.mark.parametrize("f", FAR)
def test_device_against_oracle_other_scenes(eng, f, scene, tuning):
    """70 obstacles: the generic kernel reads the raw records over two mask words.  Lanelets: boxes and rays of the lane-centre
    cost.  Sampling level 2 on jittered knots under the automatic decomposition: the planner-sized step."""
    ref_inp, out = frames.oracle_step(scene, f)
    inp = frames.hip_inputs(SCENES[scene], FRAMES[f])
    try:
        eng.set_tuning(*tuning)
        res = eng.plan_step(inp)
        info = eng.step_info()
        print(scene, f, info)
        if scene == "arc_70_obstacles":
            assert not info["grid_kernel"]
        if scene == "level2_jitter_debug":   # one launch: many lanes per candidate, obstacle stage and selection inside, tail counting
            assert info["lanes_per_candidate"] >= 4 and not info["obstacle_kernel"] and info["fused_selection"] == 1 and info["tail"] != 0, info
        compare(eng, inp, out, res, ref_inp=ref_inp, xy_tol=_xy_tol(f, out))
        assert res["best_index"] == out["result"]["best_index"] >= 0
    finally:
        _automatic(eng)


# ------------------------------------------------------------------------------------------------- b. across frames, device vs itself
_DEVICE = {}
TOPK = 16


def _device_step(e, scene, f):
    if (scene, f) not in _DEVICE:
        inp = frames.hip_inputs(frames.scene_kw(scene), FRAMES[f])
        res = e.plan_step(inp)
        cost, flags = e.costs()
        tc, ti = e.topk(TOPK)
        _DEVICE[(scene, f)] = (inp, res, cost, flags, e.bundle(), tc[0].copy(), ti[0].copy())
    return _DEVICE[(scene, f)]


@pytest.mark.parametrize("scene", ["arc_boundary", "scurve_boundary", "arc_70_obstacles", "lanelets", "level2_jitter_prod"])
@pytest.mark.parametrize("f", FAR)
def test_device_decisions_are_frame_invariant(eng, f, scene):
    """Flag words, counters, collision count, winner and top-k of the device in frame f against the device's own at NEAR (automatic
    decomposition both times): equal on every candidate the oracle decides robustly in both frames; the others -- at most 2 % --
    must be one of the outcomes the frame's oracle admits."""
    from oracle import oracle
    from tests.admissible import FRAGILE_STATE_TOL, matches_one_outcome, path_length_weight
    ref0, o0 = frames.oracle_step(scene, "NEAR")
    ref1, o1 = frames.oracle_step(scene, f)
    robust = (o0["margin"] >= FRAGILE) & (o1["margin"] >= FRAGILE)
    n_frag = int((~robust).sum())
    assert n_frag <= frames.MAX_FRAGILE_FRACTION * ref0.n_candidates, (n_frag, ref0.n_candidates)
    _, r0, c0, f0, _, tc0, ti0 = _device_step(eng, scene, "NEAR")
    inp, r1, c1, f1, planes1, tc1, ti1 = _device_step(eng, scene, f)
    assert np.array_equal(f1[robust], f0[robust]), f"{int((f1 != f0)[robust].sum())} robust candidates decided differently in {f}"
    w_pl, _ = path_length_weight(inp)
    for g in np.nonzero(~robust)[0]:
        outs = oracle.admissible_outcomes(ref1, int(g), o1["frag_sites"][g])
        st = bool(f1[g] & _abi.FX_FLAG_RETURNED) and (bool(f1[g] & _abi.FX_FLAG_COSTED) or inp.draw_traj_set)
        assert matches_one_outcome(outs, f1[g], c1[g] if f1[g] & _abi.FX_FLAG_COSTED else None, planes1[g], cost_rtol=COST_RTOL,
                                   state_tol=FRAGILE_STATE_TOL, planes_stored=st, path_length=(abs(w_pl), inp.dt)), (g, hex(int(f1[g])))
    same = np.array_equal(f1, f0)
    for k in ("n_returned", "n_feasible", "n_infeasible", "n_candidates"):
        assert r1[k] == r0[k] if same else abs(r1[k] - r0[k]) <= n_frag, k
    assert np.abs(np.array(r1["reason_hist"]) - np.array(r0["reason_hist"])).max() <= (0 if same else n_frag)
    # winner, collision count, top-k: equal -- a differing rank must be a pair whose costs at NEAR are closer than the two costs
    # moved between the frames (the reference-path tables carry the frame's rounding into every cost), or involve a fragile candidate
    moved = np.abs(c1 - c0)
    print(f"{scene} {f}: {n_frag} fragile, flag words {'equal' if same else 'differ on fragile candidates'}, costs moved by "
          f"{(moved / np.maximum(np.abs(c0), 1e-12))[(f0 & _abi.FX_FLAG_COSTED) != 0].max():.3g} relative")
    differ = np.nonzero(ti1 != ti0)[0]
    for j in differ:
        a, b = int(ti0[j]), int(ti1[j])
        assert a >= 0 and b >= 0
        assert not (robust[a] and robust[b]) or abs(c0[a] - c0[b]) <= moved[a] + moved[b], (j, a, b)
    if len(differ) == 0 or differ[0] > 0:
        assert r1["best_index"] == r0["best_index"] >= 0
        assert r1["n_collisions"] == r0["n_collisions"] or not same
        assert abs(r1["best_cost"] - r0["best_cost"]) <= moved[r0["best_index"]]


# ------------------------------------------------------------------------------------------------- c. the update path
@pytest.mark.parametrize("scene,stage", [("arc_boundary", 0), ("arc_boundary_open", 2)])
def test_update_state_equals_fresh_upload_in_utm(eng, eng2, scene, stage):
    """Five fx_update_state steps in UTM, the ego advancing 1 m per step along the reference (two knots) with the predictions
    carried along (the in-place path computes the hot table's origin a second time): each bit for bit what a fresh upload of the
    same inputs gives in another context, and each held to the oracle as in a.  Under the automatic decomposition (road
    boundary: obstacle stage fused) and on fx_obstacle_kernel, whose prediction cost carries the hot table's digits: a library
    that keeps the upload's origin differs from the fresh upload on that leg (tried, see the module's docstring)."""
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    from frenetix_motion_planner_amd.problem import pack_predictions
    from oracle import oracle
    kw, fr = frames.scene_kw(scene), FRAMES["UTM"]

    def moved(builder, j):
        inp = frames.hip_inputs(kw, fr) if builder is build_obstacle_hulls else frames.oracle_inputs(kw, fr)
        cs = inp.coordinate_system
        s0 = float(inp.x0_lon[0])
        inp.x0_lon = inp.x0_lon + np.array([1.0 * j, 0.0, 0.0])
        inp.x0_orientation = float(cs.ref_theta[cs.segment_of(float(inp.x0_lon[0]))])
        shift = cs.convert_to_cartesian_coords(s0 + 1.0 * j, 0.0) - cs.convert_to_cartesian_coords(s0, 0.0)
        preds = {k: dict(p, pos_list=np.asarray(p["pos_list"]) + shift[None, :]) for k, p in inp.predictions.items()}
        inp.obstacles = pack_predictions(preds, inp.n_samples, builder)
        inp.predictions = preds
        inp._skey = None
        return inp

    try:
        for e in (eng, eng2):
            e.set_obstacle_stage(stage)
        _update_steps(eng, eng2, kw, fr, moved, stage)
    finally:
        for e in (eng, eng2):
            e.set_obstacle_stage(0)


def _update_steps(eng, eng2, kw, fr, moved, stage):
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    from oracle import oracle
    eng.upload(frames.hip_inputs(kw, fr))
    eng.evaluate()
    eng.finish()
    winners = set()
    for j in range(1, 6):
        m = moved(build_obstacle_hulls, j)
        up = eng.make_state_update(x0_lon=m.x0_lon, x0_lat=m.x0_lat, x0_orientation=m.x0_orientation, v_des=m.v_des, v_samp=m.v_samp,
                                   obstacles=m.obstacles)
        eng.update_state(up)
        eng.evaluate()
        ra = eng.finish()[0]
        assert eng.step_info()["obstacle_kernel"] == (stage == 2)
        ca, fa = eng.costs()
        pa, ma = eng.bundle(), eng.costmap()
        rb = eng2.plan_step(m)
        assert eng2.step_info()["obstacle_kernel"] == (stage == 2)
        cb, fb = eng2.costs()
        assert np.array_equal(fa, fb) and np.array_equal(ca, cb), j
        assert np.array_equal(pa, eng2.bundle()) and np.array_equal(ma, eng2.costmap()), j
        if m.mode & _abi.FX_MODE_ROAD_BOUNDARY:
            assert np.array_equal(eng.boundary_steps(), eng2.boundary_steps()), j
        for k in RESULT_KEYS:
            assert ra[k] == rb[k], (j, k)
        ref_inp = moved(oracle.build_obstacle_hulls, j)
        out = oracle.plan_step(ref_inp)
        compare(eng2, m, out, rb, ref_inp=ref_inp, xy_tol=frames.xy_tol("UTM", _top(out)))
        assert out["collision"].sum() > 100
        winners.add(ra["best_index"])
    assert -1 not in winners


# ------------------------------------------------------------------------------------------------- d. mixed frames in one launch
def _pin_decomposition(e, info):
    """force the work decomposition step_info reports for the last launch"""
    lanes, grid = info["lanes_per_candidate"], bool(info["grid_kernel"])
    e.set_tuning(lanes, info["waves_per_simd"], 2 if grid else 1, info["block"] if grid else 0,
                 0 if lanes == 1 else (2 if info["wave_split"] else 1))
    e.set_obstacle_stage(2 if info["obstacle_kernel"] else 1, info["obstacle_steps_per_item"] if info["obstacle_kernel"] else 0)


BATCHES = {
    # automatic decomposition; road boundaries, lanelets (no obstacles) and a debug flag set in one launch
    "automatic": (0, [("scurve_boundary", "NEAR"), ("level2_jitter_debug", "KM"), ("lanelets", "UTM"), ("arc_boundary", "UTM2")]),
    # fx_obstacle_kernel behind the walk (its prediction cost carries the hot table's digits): an agent's table read against another
    # agent's origin would be kilometres off
    "obstacle_kernel": (2, [("scurve_boundary_open", "UTM"), ("level2_jitter_debug", "KM"), ("no_obstacles", "UTM2"), ("arc_boundary_open", "NEAR"),
                            ("arc_boundary_open", "UTM2")]),
}


def _batch_kw(name):
    return dict(frames.scene_kw("scurve_boundary_open"), n_obstacles=0) if name == "no_obstacles" else frames.scene_kw(name)


@pytest.mark.parametrize("which", sorted(BATCHES))
def test_agents_in_four_frames_in_one_launch(which):
    """One batched evaluate over agents at NEAR, KM, UTM and UTM2, with and without obstacles (every agent has its own hot-table
    origin): each agent held to its oracle, and bit for bit the same agent run alone under the batch's decomposition."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    stage, agents = BATCHES[which]
    assert {f for _, f in agents} == set(FRAMES)
    inps = [frames.hip_inputs(_batch_kw(s), FRAMES[f]) for s, f in agents]
    assert not all(i.obstacles["K"] > 0 for i in inps) and sum(i.obstacles["K"] > 0 for i in inps) >= 3
    with FrenetEngine(max_candidates=24_000, max_steps=40, max_ref_knots=512, max_obstacles=32, max_pred_steps=64, max_agents=len(inps)) as eng:
        eng.set_obstacle_stage(stage)
        res = eng.plan_batch(inps)
        info = eng.step_info()
        assert info["agents"] == len(inps) and info["obstacle_kernel"] == (stage == 2)
        batch = []
        for a, (s, f) in enumerate(agents):
            if s == "no_obstacles":
                ref_inp = frames.oracle_inputs(_batch_kw(s), FRAMES[f])
                out = oracle.plan_step(ref_inp)
            else:
                ref_inp, out = frames.oracle_step(s, f)
            compare(eng, inps[a], out, res[a], agent=a, ref_inp=ref_inp, xy_tol=_xy_tol(f, out))
            batch.append((*eng.costs(a), eng.costmap(a), eng.bundle(a)))
        _pin_decomposition(eng, info)
        for a, inp in enumerate(inps):
            r = eng.plan_step(inp)
            one = eng.step_info()
            assert all(one[k] == info[k] for k in ("lanes_per_candidate", "grid_kernel", "wave_split")), (agents[a], one, info)
            assert one["obstacle_kernel"] == info["obstacle_kernel"] or not inp.obstacles["K"], (agents[a], one, info)
            cost, flags = eng.costs()
            assert np.array_equal(batch[a][1], flags) and np.array_equal(batch[a][0], cost), agents[a]
            assert np.array_equal(batch[a][2], eng.costmap()) and np.array_equal(batch[a][3], eng.bundle()), agents[a]
            for k in RESULT_KEYS:
                assert res[a][k] == r[k], (agents[a], k)


# ------------------------------------------------------------------------------------------------- e. consumers of the step, in UTM
def _utm_kw():
    return frames.place(SCENES["arc_boundary"], FRAMES["UTM"])


def test_materialise_and_read_back_in_utm(eng):
    """materialise of the winner and the top 8 behind a select-only step: the rows of the bundle-mode twin, bit for bit
    (test_materialise_gpu at the origin); the batched read-back equals the single ones."""
    from tests.test_materialise_gpu import assert_rows_equal, bundle_twin, select_only
    from tests.test_read_candidates import assert_same, singles
    kw = _utm_kw()
    inp_b, res_b, want = bundle_twin(eng, kw)
    ids = np.random.default_rng(3).permutation(inp_b.n_candidates)[:70]
    assert_same(eng.candidates(ids), singles(eng, ids))
    inp = select_only(kw)
    res = eng.plan_step(inp)
    assert res["best_index"] == res_b["best_index"] >= 0
    _, ti = eng.topk(8)
    ids = np.concatenate([[res["best_index"]], ti[0][ti[0] >= 0]]).astype(np.int64)
    assert len(ids) == 9
    cost, flags = eng.costs()
    got = eng.materialise(ids)
    assert_rows_equal(got, want, ids, inp_b, boundary=True)
    assert np.array_equal(got["flags"], flags[ids]) and np.allclose(got["cost"], cost[ids], rtol=1e-12, atol=0)
    assert np.abs(got["planes"][:, :2]).max() > 5e6


def test_winner_package_in_utm(eng):
    ref_inp, out = frames.oracle_step("arc_boundary", "UTM")
    inp = frames.hip_inputs(SCENES["arc_boundary"], FRAMES["UTM"])
    eng.set_package(True)
    try:
        res = eng.plan_step(inp)
        pkg = eng.package(0, 0.125)
        cost, _ = eng.costs()
        assert pkg is not None and pkg.index == res["best_index"] == out["result"]["best_index"]
        assert pkg.cost == cost[pkg.index] == res["best_cost"]
        assert np.array_equal(pkg.block[:_abi.FX_NUM_PLANES], eng.sample(pkg.index))
        assert np.abs(pkg.block[:2] - out["planes"][pkg.index][:2]).max() < frames.xy_tol("UTM", _top(out))
    finally:
        eng.set_package(False)


@pytest.fixture(scope="module")
def utm_step(eng):
    inp = frames.hip_inputs(SCENES["arc_boundary"], FRAMES["UTM"])
    eng.plan_step(inp)
    _, flags = eng.costs()
    planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
    return eng, inp, flags, planes


@pytest.mark.parametrize("maha", [False, True])
def test_risk_in_utm(utm_step, maha):
    """risk() in the default and the Mahalanobis mode on the device's own read-back planes (test_risk_gpu's obstacles, which walk
    along ego candidates: here at 5e6 m) against the restatement, at that module's tolerance"""
    from frenetix_motion_planner_amd import risk
    from tests import risk_restatement as rr
    from tests.test_risk_gpu import BASE, EGO, HARM, _predictions
    eng, inp, flags, planes = utm_step
    modes = dict(BASE, fast_prob_mahalanobis=maha)
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), zero_cov=not maha)
    tabs = risk.obstacle_tables(preds, typ, mahalanobis=maha)
    eng.set_risk_obstacles(tabs)
    ego, obst, idx = eng.risk(risk.risk_params(modes, HARM, **EGO))
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    assert len(ids) > 100
    we, wo = rr.calc_risk(planes["x"][ids], planes["y"][ids], planes["theta"][ids], planes["v"][ids], preds, typ, modes, HARM, **EGO)
    assert (we > 0).sum() > len(ids) // 4, "too few candidates near an obstacle"
    for got, want in ((ego[ids], we), (obst[ids], wo)):
        err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
        print(f"risk, mahalanobis={maha}: {err.max():.2e}")
        assert err.max() < 1e-12, err.max()
    assert idx == rr.min_risk_index(ego[ids], obst[ids], ids)


def test_risk_costs_in_utm(utm_step):
    """risk_costs() with the action-space responsibility against tests/risk_costs_restatement.py, at test_risk_costs_gpu's tolerances"""
    from frenetix_motion_planner_amd import risk
    from tests import risk_costs_restatement as rcr
    from tests.test_risk_costs_gpu import COEFF, COLS, WEIGHTS, _err
    from tests.test_risk_gpu import BASE, EGO, HARM, _predictions
    eng, inp, flags, planes = utm_step
    K, C = 8, inp.n_candidates
    preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=K)
    eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
    params = risk.risk_params(BASE, HARM, **EGO)
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    sub = ids[::3]
    x0 = np.array([planes["x"][ids[0], 0], planes["y"][ids[0], 0]])
    th0 = float(planes["theta"][ids[0], 0]) + 0.5
    bh = np.where(np.random.default_rng(5).random(C) < 0.4, 1.0 / (1.0 + np.exp(-COEFF[0] - COEFF[1] * planes["v"][:, 7])), 0.0)
    resp = risk.action_space_responsibility(preds, x0, th0)
    assert 0 < resp.sum() < K
    P = [planes[n][sub] for n in ("x", "y", "theta", "v")]
    want = rcr.calc_risk_detail(*P, preds, typ, BASE, HARM, **EGO)
    assert (want["ego_risk"] > 0).sum() > len(sub) // 4
    part = eng.risk_costs(params, risk.risk_cost_params(WEIGHTS, boundary_harm=bh[sub], responsibility=resp), sub)
    for q in COLS + ("ego_risk", "obst_risk", "obst_harm_occ"):
        assert _err(part[q], want[q]) < 1e-12, (q, _err(part[q], want[q]))
    wr = [rcr.responsibility_action_space(want["obst_risk_max"][c], preds, x0, th0) for c in range(len(sub))]
    wc = rcr.costs(want, bh[sub], WEIGHTS, wr)
    tol = dict(bayes=(2 * K + 1) * 1e-12, equality=(2 * K + 1) * 1e-12, maximin=10e-12, ego=(2 * K + 1) * 1e-12,
               responsibility=(2 * K + 1) * 1e-12)
    tol["total"] = sum(w * tol[n] for w, n in zip(WEIGHTS, rcr.NAMES))
    for q, t in tol.items():
        print(f"risk_costs {q}: {_err(part[q], wc[q]):.2e} (bound {t:.1e})")
        assert _err(part[q], wc[q]) < t, q
    assert part["min_cost_index"] == rcr.argmin_index(part["total"], sub)
