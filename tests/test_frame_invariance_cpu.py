"""Away from the world origin, on the CPU (tests/frames.py names the frames and the scenes; DESIGN.md section 2 "Away from the origin").

The oracle brute-forces every (candidate, obstacle, boundary piece) pair on absolute coordinates and has no hot table, no origin
and no bins: if ITS decisions are the same in every frame it is a usable reference in every frame, and an exact cross-frame
comparison of decisions is a fair demand on the device (tests/test_frame_invariance_gpu.py).  Its numbers do move between frames
-- the host's reference-path tables are built from differences of absolute coordinates -- and by how much is MEASURED here
(`python -m tests.test_frame_invariance_cpu` writes profiles/frames/oracle_frames.json), not asserted against a constant
chosen in advance; what is asserted about numbers follows from np.spacing of the operands, the reasoning written at each bound.
"""
import json
import os

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, synthetic
from frenetix_motion_planner_amd.coordinate_system import CoordinateSystem
from tests import frames
from tests.frames import FAR, FRAMES, SCENES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "frames", "oracle_frames.json")
ALL_SCENES = sorted(SCENES) + ["level2_jitter_prod"]


# ------------------------------------------------------------------------------------------------- placed inputs
def _arrays(inp):
    """every array and scalar the library, the oracle or a test reads from a PlanInputs"""
    cs = inp.coordinate_system
    out = dict(reference=cs.reference, ref_pos=cs.ref_pos, ref_theta=cs.ref_theta, ref_curv=cs.ref_curv, ref_curv_d=cs.ref_curv_d,
               normals=cs.normals, x0_lon=inp.x0_lon, x0_lat=inp.x0_lat, x0_orientation=np.float64(inp.x0_orientation),
               v_des=np.float64(inp.v_des))
    for k in ("t_samp", "v_samp", "d_samp", "sampling_matrix"):
        if getattr(inp, k) is not None:
            out[k] = np.asarray(getattr(inp, k))
    for k, v in (inp.obstacles or {}).items():
        if isinstance(v, np.ndarray):
            out["obstacles." + k] = v
    if inp._bound is not None:
        for k in ("piece", "bin", "item"):
            out["bound." + k] = inp._bound[k]
        out["bound.reach"] = np.float64(inp._bound["reach"])
    if inp.road_boundary is not None and isinstance(inp.road_boundary, np.ndarray):
        out["road_boundary"] = inp.road_boundary
    for k, p in (inp.predictions or {}).items():
        out[f"pred.{k}.pos"], out[f"pred.{k}.yaw"] = np.asarray(p["pos_list"]), np.asarray(p["orientation_list"])
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.parametrize("name", ["dense_prod_obs", "lane_center", "proj_pseudo_bisector_prod"])
def test_default_origin_leaves_the_inputs_bit_identical(name):
    """make_inputs without `origin` (what bench.py, smoke() and every other test call), with the default spelled out and with
    a signed zero: the same bits in every array -- and the reference is reference_polyline()'s own array, nothing added to it."""
    from tests.test_hip_parity import CASES
    kw = dict(CASES[name], road_half_width=3.0)
    base = _arrays(synthetic.make_inputs(**kw))
    want_ref = synthetic.reference_polyline(kw["ref_kind"], 400, 0.5, kw.get("kappa", 0.01), kw.get("knot_jitter", 0.0), synthetic.SEED,
                                            0.0)
    assert np.array_equal(_bits(base["reference"]), _bits(want_ref))
    for origin in ((0.0, 0.0), (0, 0), (-0.0, 0.0)):
        got = _arrays(synthetic.make_inputs(origin=origin, **kw))
        assert got.keys() == base.keys()
        for k, w in base.items():
            assert np.array_equal(_bits(got[k]), _bits(w)), (origin, k)
    moved = _arrays(synthetic.make_inputs(origin=(1000.0, -2000.0), **kw))
    assert np.array_equal(moved["reference"], want_ref + np.array([1000.0, -2000.0]))   # translated AFTER heading0, nothing else
    assert np.array_equal(moved["t_samp"], base["t_samp"]) and np.array_equal(moved["d_samp"], base["d_samp"])


def test_frames_carry_the_polyline_rigidly():
    """heading0 + origin is the rigid motion frames.carry_points states: rotation about the first knot, then the translation"""
    for f in FAR:
        kw = SCENES["scurve_boundary"]
        near = frames.oracle_inputs(kw).coordinate_system.reference
        far = frames.oracle_inputs(kw, FRAMES[f]).coordinate_system.reference
        assert np.abs(far - frames.carry_points(near, FRAMES[f])).max() <= 4 * np.spacing(frames.magnitude(FRAMES[f]))
        assert np.abs(far).max() > 0.9 * max(abs(FRAMES[f][0][0]), abs(FRAMES[f][0][1]))


# ------------------------------------------------------------------------------------------------- the oracle across frames
def _deviation(scene, f):
    """numeric deviation of the oracle in frame f from its own NEAR answers carried into f (stored candidates)"""
    inp0, o0 = frames.oracle_step(scene, "NEAR")
    inp1, o1 = frames.oracle_step(scene, f)
    st = frames.stored(inp0, o0)
    want = frames.carry_planes(o0["planes"][st], FRAMES[f])
    got = o1["planes"][st]
    top = float(np.abs(got[:, :2]).max())
    d = np.abs(got - want)
    rel = d / (1.0 + np.abs(want).max(axis=2, keepdims=True))
    c = o0["costed"]
    dc = np.abs(o1["cost"][c] - o0["cost"][c]) / np.maximum(np.abs(o0["cost"][c]), 1e-12)
    dm = np.abs(o1["costmap"][c] - o0["costmap"][c]) / np.maximum(np.abs(o0["costmap"][c]), 1e-9)
    return dict(xy_vs_near_ulps=float(d[:, :2].max() / np.spacing(top)), theta=float(d[:, 2].max()),
                other_planes=float(rel[:, 3:].max()), cost=float(dc.max()) if c.any() else 0.0,
                costmap=float(dm.max()) if c.any() and dm.size else 0.0, max_coordinate=top)


@pytest.mark.parametrize("f", FAR)
@pytest.mark.parametrize("scene", ALL_SCENES)
def test_oracle_decisions_are_frame_invariant(scene, f):
    inp0, o0 = frames.oracle_step(scene, "NEAR")
    inp1, o1 = frames.oracle_step(scene, f)
    assert inp0.n_candidates == inp1.n_candidates
    for k in ("flags", "collision", "boundary_step", "reasons", "selectable", "traj_len", "frag_sites"):
        assert np.array_equal(o1[k], o0[k]), k
    for k in ("best_index", "n_collisions", "n_returned", "n_feasible", "reason_hist", "n_candidates"):
        assert o1["result"][k] == o0["result"][k], k
    robust = (o0["margin"] >= frames.FRAGILE) & (o1["margin"] >= frames.FRAGILE)
    assert np.array_equal(o0["margin"] >= frames.FRAGILE, o1["margin"] >= frames.FRAGILE)
    # the stable cost order of the robust candidates: equal, except between neighbours whose costs at NEAR are closer than the two
    # costs moved between the frames (a swap of a and b needs |c(a) - c(b)| <= |dc(a)| + |dc(b)|)
    a = np.array([g for g in o0["order"] if g >= 0 and robust[g]])
    b = np.array([g for g in o1["order"] if g >= 0 and robust[g]])
    assert len(a) == len(b) and np.array_equal(np.sort(a), np.sort(b))
    moved = np.abs(o1["cost"] - o0["cost"])
    for j in np.nonzero(a != b)[0]:
        assert abs(o0["cost"][a[j]] - o0["cost"][b[j]]) <= moved[a[j]] + moved[b[j]], (j, a[j], b[j])
    assert (a != b).sum() <= 0.01 * max(len(a), 200)
    dev = _deviation(scene, f)
    print(f"{scene} {f}: " + ", ".join(f"{k} {v:.3g}" for k, v in dev.items()))
    # the scenes are what the module says they are
    assert o0["result"]["best_index"] >= 0
    if scene != "level2_jitter_debug":
        assert (~robust).sum() <= frames.MAX_FRAGILE_FRACTION * inp0.n_candidates


def test_scenes_keep_collisions_and_off_road_candidates_well_represented():
    for scene, n_coll, n_off in (("arc_boundary", 1000, 200), ("scurve_boundary", 400, 50), ("arc_70_obstacles", 200, 0),
                                 ("level2_jitter_debug", 5, 0)):
        inp, out = frames.oracle_step(scene, "NEAR")
        assert out["collision"].sum() >= n_coll and out["boundary"].sum() >= n_off, scene
        assert out["result"]["n_collisions"] > 0 or scene == "level2_jitter_debug"
    inp, _ = frames.oracle_step("arc_70_obstacles", "NEAR")
    assert inp.obstacles["K"] == 70                      # raw records over two mask words
    inp, _ = frames.oracle_step("lanelets", "NEAR")
    assert "lane_center_offset" in inp.cost_names and inp.lanelets is not None


# ------------------------------------------------------------------------------------------------- independent projection
@pytest.mark.parametrize("f", sorted(FRAMES))
def test_oracle_projection_against_extended_precision(f):
    """The oracle's (x, y) against DESIGN 4.1 restated in np.longdouble on the oracle's own (s, d).  Evaluating p + d n / |n| in
    doubles takes ~9 roundings whose results are of the coordinates' magnitude or feed one that is (two interpolations, the
    product d n, the sum), each at most half a spacing of the largest coordinate: more than 5 spacings would be an arithmetic error, not
    rounding.  The measured figure (about 1) is what the GPU module's xy tolerance is built from."""
    worst = max(frames.oracle_xy_error_ulps(scene, f)[0] for scene in SCENES)
    print(f"{f}: oracle (x, y) within {worst:.3f} spacings of the extended-precision projection; n = {frames.xy_ulps_allowed(f)}")
    assert worst <= 5.0
    assert frames.xy_ulps_allowed(f) == 2 * int(np.ceil(worst))


def test_extended_projection_is_not_the_oracles_code():
    """... and it agrees with the host's own forward map (a third implementation) the same way: a mistake in the restatement
    would show here at once"""
    cs = frames.oracle_inputs(SCENES["level2_jitter_debug"], frames.UTM).coordinate_system
    rng = np.random.default_rng(5)
    s = rng.uniform(cs.ref_pos[0], cs.ref_pos[-1], 500)
    d = rng.uniform(-4.0, 4.0, 500)
    ex, ey, valid = frames.project_extended(cs, s, d)
    assert valid.all()
    host = np.array([cs.convert_to_cartesian_coords(float(a), float(b)) for a, b in zip(s, d)])
    err = np.maximum(np.abs(host[:, 0] - ex), np.abs(host[:, 1] - ey)).max()
    assert err <= 5 * np.spacing(np.abs(host).max())
    _, _, valid = frames.project_extended(cs, np.array([cs.ref_pos[0] - 1e-9, cs.ref_pos[-1] + 1e-9]), np.zeros(2))
    assert not valid.any()


# ------------------------------------------------------------------------------------------------- compare()'s absolute (x, y) bound
def test_xy_tol_notices_what_the_relative_bound_lets_through():
    """compare() holds the planes relative to 1 + their peak: at UTM an x plane off by 1e-6 m (a thousand spacings) passes.  With
    xy_tol -- the absolute bound the GPU module passes in the UTM frames -- it fails, and the unperturbed answer passes."""
    from tests.oracle_engine import OracleEngine
    from tests.test_hip_parity import compare

    class Engine(OracleEngine):
        shift = 0.0

        def bundle(self, agent=0):
            planes = self.last[agent][1]["planes"].copy()
            planes[self.victim, 0, 3:] += self.shift
            return planes

        def sample(self, index, agent=0):
            return self.bundle(agent)[index]

    inp, out = frames.oracle_step("lanelets", "UTM")
    eng = Engine()
    res = eng.plan_step(inp)
    eng.victim = int(np.nonzero(frames.stored(inp, out) & (out["margin"] >= frames.FRAGILE))[0][7])
    tol = frames.xy_tol("UTM", float(np.abs(out["planes"][:, :2]).max()))
    assert 1e-9 < tol < 4e-9
    compare(eng, inp, out, res, xy_tol=tol)
    eng.shift = 1e-6
    compare(eng, inp, out, res)
    with pytest.raises(AssertionError, match="off by"):
        compare(eng, inp, out, res, xy_tol=tol)
    eng.shift = 2.5 * tol
    with pytest.raises(AssertionError, match="off by"):
        compare(eng, inp, out, res, xy_tol=tol)


# ------------------------------------------------------------------------------------------------- host maps in every frame
READINGS = [(False, "chord"), (True, "chord"), (False, "bisector"), (True, "bisector")]


def _polyline(frame):
    (ox, oy), angle = frame
    p = synthetic.reference_polyline("arc", 300, 0.5, 0.03, 0.3, synthetic.SEED, angle)
    return p + np.array([ox, oy])[None, :] if (ox or oy) else p


@pytest.mark.parametrize("pseudo,tangent", READINGS)
@pytest.mark.parametrize("f", sorted(FRAMES))
def test_host_maps_round_trip_in_every_frame(f, pseudo, tangent):
    """convert_to_cartesian_coords -> convert_to_curvilinear_coords returns (s, d), and frenet_state of the carried vehicle state
    is NEAR's, in every frame and projection reading.  Bounds, with u = np.spacing(largest coordinate), h = shortest knot spacing:
      * (s, d): the forward map rounds (x, y) to within 5 u (above); the inverse forms differences of absolute coordinates
        (each exact or within u), and a point error e moves (s, d) by at most e / (1 - kappa d) <= 1.2 e here (kappa 0.03,
        |d| <= 3.5, jittered knots); the vertex normals, from differences of knots that each carry u / 2, turn by <= 2 u / h and
        move a point at |d| <= 3.5 by 7 u / h.  Sum: (12 + 7 / h) u, on top of the 1e-8 that test_host_logic.py's
        test_coordinate_system_roundtrip holds the inverse map's own quadratic solve to at the origin (measured here: 3.5e-10
        at NEAR, 7.9e-10 at UTM -- the inverse takes its differences against the point first and does not feel the frame).
      * s', d', s'', d'': functions of theta_ref (atan2 of knot differences: <= 2 u / h), kappa_ref (second differences:
        <= 8 u / h^2 ... np.gradient twice) and kappa_ref' (one more difference over h: 16 u / h^3), multiplied by at most
        v^2 (1 + |d|) = 500 here."""
    fr = FRAMES[f]
    cs = CoordinateSystem(_polyline(fr), pseudo_normal=pseudo, vertex_tangent=tangent)
    near = CoordinateSystem(_polyline(frames.NEAR), pseudo_normal=pseudo, vertex_tangent=tangent)
    u = float(np.spacing(np.abs(cs.reference).max()))
    h = float(np.diff(cs.ref_pos).min())
    rng = np.random.default_rng(11)
    s = rng.uniform(cs.ref_pos[2], cs.ref_pos[-3], 200)
    d = rng.uniform(-3.5, 3.5, 200)
    tol_sd = (12.0 + 7.0 / h) * u + 1e-8
    worst = 0.0
    for a, b in zip(s, d):
        xy = cs.convert_to_cartesian_coords(float(a), float(b))
        back = cs.convert_to_curvilinear_coords(float(xy[0]), float(xy[1]))
        worst = max(worst, abs(back[0] - a), abs(back[1] - b))
    print(f"{f} pseudo_normal={pseudo} {tangent}: (s, d) round trip {worst:.3g} (bound {tol_sd:.3g})")
    assert worst <= tol_sd
    tol_dyn = 500.0 * (2.0 / h + 8.0 / h ** 2 + 16.0 / h ** 3) * u + 1e-10
    worst_sd = worst_dyn = 0.0
    for a, b in zip(s[:60], d[:60]):
        k = near.segment_of(float(a))
        xy0 = near.convert_to_cartesian_coords(float(a), float(b))
        heading, speed, acc, curv = float(near.ref_theta[k]) + 0.1, 9.0, -0.7, 0.02
        xy1 = frames.carry_points(xy0, fr)
        for arc in (False, True):
            lon0, lat0 = near.frenet_state(xy0[0], xy0[1], heading, speed, acc, curv, arc)
            lon1, lat1 = cs.frenet_state(xy1[0], xy1[1], heading + fr[1], speed, acc, curv, arc)
            worst_sd = max(worst_sd, abs(lon1[0] - lon0[0]), abs(lat1[0] - lat0[0]))
            worst_dyn = max(worst_dyn, *(abs(p - q) for p, q in zip(lon1[1:] + lat1[1:], lon0[1:] + lat0[1:])))
    print(f"{f} pseudo_normal={pseudo} {tangent}: frenet_state vs NEAR (s, d) {worst_sd:.3g} (bound {2 * tol_sd:.3g}), "
          f"derivatives {worst_dyn:.3g} (bound {tol_dyn:.3g})")
    assert worst_sd <= 2 * tol_sd       # (the carried point is itself rounded once more, and NEAR's own round trip counts)
    assert worst_dyn <= tol_dyn


@pytest.mark.parametrize("f", sorted(FRAMES))
@pytest.mark.parametrize("scene", ["arc_boundary", "scurve_boundary"])
def test_boundary_bins_hold_every_piece_within_reach(scene, f):
    """The broad phase at large coordinates: for EVERY knot k, every piece that the brute force finds touching an ego
    footprint whose foot point lies on reference segment k -- footprints at the segment's ends and middle, laterally across
    +-bound_d_reach, at headings up to 0.6 rad off the reference's -- is listed in bin k."""
    inp, _ = frames.oracle_step(scene, f)
    bd, cs, veh = inp._bound, inp.coordinate_system, inp.vehicle
    piece = bd["piece"]
    hl, hw = veh.length / 2, veh.width / 2
    M = len(cs.reference)
    lam = np.array([0.0, 0.5, 1.0])
    dd = np.linspace(-bd["d_reach"], bd["d_reach"], 9)
    dth = np.array([-0.6, 0.0, 0.6])
    seg = cs.reference[1:] - cs.reference[:-1]
    th_ref = np.arctan2(seg[:, 1], seg[:, 0])
    nrm = np.stack([-np.sin(th_ref), np.cos(th_ref)], axis=1)
    n_touch = 0
    for k in range(M - 1):
        foot = cs.reference[k][None, :] + lam[:, None] * seg[k][None, :]                           # [3, 2]
        rear = (foot[:, None, :] + dd[None, :, None] * nrm[k][None, None, :]).reshape(-1, 2)       # [27, 2]
        th = th_ref[k] + dth                                                                       # [3]
        u = np.stack([np.cos(th), np.sin(th)], axis=1)                                             # [3, 2]
        c = (rear[:, None, :] + veh.wb_rear_axle * u[None, :, :]).reshape(-1, 2)                   # [81, 2]
        uu = np.tile(u, (len(rear), 1))
        nn = np.stack([-uu[:, 1], uu[:, 0]], axis=1)
        # (pieces farther than three times the reach from the knot cannot touch: every footprint point is within
        # segment + d_reach + wb_rear_axle + half diagonal of it by the triangle inequality -- they are left out for speed only)
        cand = np.nonzero(np.linalg.norm(piece[:, :2] - cs.reference[k], axis=1) <= 3.0 * bd["reach"] + 2.0)[0]
        pc = piece[cand]
        e = pc[None, :, :2] - c[:, None, :]                                                        # [81, n, 2]
        ex, ey = (e * uu[:, None, :]).sum(-1), (e * nn[:, None, :]).sum(-1)
        hx, hy = pc[:, 2:] @ uu.T, pc[:, 2:] @ nn.T                                                # [n, 81]
        hx, hy = hx.T, hy.T
        sep = (np.abs(ex) > hl + np.abs(hx)) | (np.abs(ey) > hw + np.abs(hy)) | (np.abs(ex * hy - ey * hx) > hl * np.abs(hy) + hw * np.abs(hx))
        touching = cand[np.nonzero((~sep).any(axis=0))[0]]
        n_touch += len(touching)
        in_bin = set(bd["item"][bd["bin"][k]:bd["bin"][k + 1]].tolist())
        assert set(touching.tolist()) <= in_bin, (k, sorted(set(touching.tolist()) - in_bin))
    assert n_touch > M                                                                            # (not a comparison of empty sets)
    # ... and the bins are the NEAR frame's: a rigid motion changes no distance by more than rounding
    near = frames.oracle_step(scene, "NEAR")[0]._bound
    assert np.array_equal(bd["bin"], near["bin"]) and np.array_equal(bd["item"], near["item"])


# ------------------------------------------------------------------------------------------------- the written record
def measure():
    out = dict(frames={k: dict(origin=list(v[0]), angle=v[1]) for k, v in FRAMES.items()}, scenes={}, xy={})
    for f in sorted(FRAMES):
        per = {scene: frames.oracle_xy_error_ulps(scene, f)[0] for scene in SCENES}
        out["xy"][f] = dict(oracle_vs_extended_precision_spacings=max(per.values()), per_scene=per, n=frames.xy_ulps_allowed(f))
    for scene in ALL_SCENES:
        inp, o = frames.oracle_step(scene, "NEAR")
        out["scenes"][scene] = dict(candidates=int(inp.n_candidates), collisions=int(o["collision"].sum()), off_road=int(o["boundary"].sum()),
                                    winner=int(o["result"]["best_index"]), fragile=int((o["margin"] < frames.FRAGILE).sum()),
                                    deviation_from_near={f: _deviation(scene, f) for f in FAR})
    return out


def test_profile_names_every_scene_and_frame():
    rec = json.load(open(PROFILE))
    assert set(rec["scenes"]) == set(ALL_SCENES) and set(rec["xy"]) == set(FRAMES)
    for scene in ALL_SCENES:
        assert set(rec["scenes"][scene]["deviation_from_near"]) == set(FAR)
        assert rec["scenes"][scene]["candidates"] == frames.oracle_step(scene, "NEAR")[0].n_candidates
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Away from the origin" in design and "profiles/frames/oracle_frames.json" in design
    assert "recentre" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


if __name__ == "__main__":
    os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
    with open(PROFILE, "w") as fh:
        json.dump(measure(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", PROFILE)
