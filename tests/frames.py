"""World frames of the frame-invariance tests: a scene built at the world origin and the same scene kilometres away.

A frame is ((origin x, origin y), angle): the synthetic reference is rotated about its first knot by `angle` (on top of the
scene's own heading0) and that knot is then moved to `origin`.  Ego state, predictions, road boundary and lanelets follow
through the CoordinateSystem (synthetic.make_inputs), so the Frenet-side problem -- sampling ranges, (s, d), every decision -- is
the same in every frame and only the Cartesian operands grow:

  NEAR   the frame every other test of the suite lives in
  KM     a CommonRoad map some kilometres from its origin
  UTM    an OSM-derived map in UTM coordinates (x ~ 7e5 m, y ~ 5e6 m: np.spacing(5.3e6) = 9.3e-10 m)
  UTM2   large coordinates of the other signs, heading near -pi
"""
import numpy as np

NEAR = ((0.0, 0.0), 0.0)
KM = ((12345.678, -9876.543), 0.7)
UTM = ((-691608.13, 5334760.77), 2.1)
UTM2 = ((4.2e5, -3.1e5), -2.9)
FRAMES = dict(NEAR=NEAR, KM=KM, UTM=UTM, UTM2=UTM2)
FAR = ("KM", "UTM", "UTM2")

PLANE_X, PLANE_Y, PLANE_THETA = 0, 1, 2


def place(kw: dict, frame) -> dict:
    """keyword arguments of synthetic.make_inputs for the scene `kw` in `frame`"""
    (ox, oy), angle = frame
    return dict(kw, heading0=kw.get("heading0", 0.0) + angle, origin=(ox, oy))


def magnitude(frame, extent: float = 400.0) -> float:
    """largest |coordinate| a scene of `extent` metres can reach in the frame"""
    (ox, oy), _ = frame
    return max(abs(ox), abs(oy)) + extent


def carry_points(xy, frame):
    """points [..., 2] of the NEAR frame carried into `frame` (rotation about the world origin -- where NEAR's first reference
    knot lies -- then the translation)"""
    (ox, oy), angle = frame
    xy = np.asarray(xy, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    return np.stack([c * xy[..., 0] - s * xy[..., 1] + ox, s * xy[..., 0] + c * xy[..., 1] + oy], axis=-1)


def carry_planes(planes, frame):
    """Oracle planes [..., 14, S] of the NEAR frame as they read in `frame`: (x, y) rotated and translated, the global heading
    theta shifted by the angle, every curvilinear / kinematic plane as it is.  Steps outside the projection domain carry
    x = y = 0 in every frame (the reference's loop breaks there) and stay so; their heading is the carried-over one
    of the last step inside and moves with the frame like any other."""
    (ox, oy), angle = frame
    out = np.array(planes, dtype=np.float64, copy=True)
    x, y = out[..., PLANE_X, :], out[..., PLANE_Y, :]
    inside = (x != 0.0) | (y != 0.0)
    moved = carry_points(np.stack([x, y], axis=-1), frame)
    out[..., PLANE_X, :] = np.where(inside, moved[..., 0], 0.0)
    out[..., PLANE_Y, :] = np.where(inside, moved[..., 1], 0.0)
    out[..., PLANE_THETA, :] = out[..., PLANE_THETA, :] + angle
    return out


# ---------------------------------------------------------------------------------------------------------------- scenes
# Small scenes with every stage that reads Cartesian operands: predictions (prediction cost + OBB collision), a road boundary
# with off-road candidates, more than 64 obstacles (raw records over two mask words: generic kernel), lanelets (lane-centre
# cost), jittered knots at sampling level 2 (the planner-sized one-launch step).  Each has a winner, colliding candidates
# in front of it where it has obstacles, and at most 2 % candidates the oracle decides by the last ulp -- except the
# debug-flag scene (every candidate keeps its planes: 70 of 630), whose production-flag twin stands in where the cap is asserted.
_LANE_COSTS = dict(lane_center_offset=2.0, lateral_jerk=0.2, velocity_offset=1.0, prediction=0.2, distance_to_reference_path=1.0)
SCENES = {
    "arc_boundary": dict(ref_kind="arc", grid=(9, 21, 21), n_obstacles=12, lead_gap=20.0, road_half_width=3.4),
    "scurve_boundary": dict(ref_kind="scurve", kappa=0.03, v0=8.0, grid=(7, 15, 17), n_obstacles=20, seed=4, road_half_width=2.6,
                            obstacle_min_gap=8.0),
    "arc_70_obstacles": dict(ref_kind="arc", grid=(5, 9, 13), n_obstacles=70, lead_gap=18.0, obstacle_min_gap=40.0),
    "lanelets": dict(ref_kind="arc", v0=9.0, grid=(4, 7, 9), lanelets=(3.5, 60), cost_weights=_LANE_COSTS),
    "level2_jitter_debug": dict(ref_kind="arc", v0=12.0, level=2, n_obstacles=5, knot_jitter=0.3, draw_traj_set=True,
                                kinematic_debug=True),
}
LEVEL2_PROD = dict(SCENES["level2_jitter_debug"], draw_traj_set=False, kinematic_debug=False)


def scene_kw(name: str) -> dict:
    """SCENES[name]; "level2_jitter_prod": the debug-flag scene under the production flag set; "<scene>_open": the scene without
    its road boundary (fx_obstacle_kernel does not run behind a walk with the road-boundary stage: the library declines)"""
    if name == "level2_jitter_prod":
        return LEVEL2_PROD
    if name.endswith("_open"):
        return {k: v for k, v in SCENES[name[:-len("_open")]].items() if k != "road_half_width"}
    return SCENES[name]
MAX_FRAGILE_FRACTION = 0.02
FRAGILE = 1e-9   # oracle margin below which a decision is taken by the last ulp (oracle.FRAGILE, tests/admissible.py)


def oracle_inputs(kw, frame=NEAR):
    from frenetix_motion_planner_amd import synthetic
    from oracle import oracle
    return synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **place(kw, frame))


def hip_inputs(kw, frame=NEAR, **more):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return synthetic.make_inputs(hull_builder=build_obstacle_hulls, **dict(place(kw, frame), **more))


_ORACLE = {}


def oracle_step(scene: str, frame: str):
    """(inputs, oracle.plan_step(inputs)) of a named scene in a named frame, computed once per process and left unchanged"""
    key = (scene, frame)
    if key not in _ORACLE:
        from oracle import oracle
        inp = oracle_inputs(scene_kw(scene), FRAMES[frame])
        _ORACLE[key] = (inp, oracle.plan_step(inp))
    return _ORACLE[key]


def stored(inp, out):
    """candidates whose planes the oracle defines (those test_hip_parity.compare holds the device to)"""
    return out["returned"] & (out["costed"] | bool(inp.draw_traj_set))


# ------------------------------------------------------------------------------------- DESIGN 4.1, restated in extended precision
def project_extended(cs, s, d):
    """DESIGN.md 4.1 from its text, in np.longdouble (64-bit significand on x86: 11 bits below a double's last): for arc
    lengths s and offsets d (float64 arrays of one shape) the point p + d n / |n| with k = clamp(upper_bound(ref_pos, s) - 1,
    0, M - 2), lambda = (s - ref_pos[k]) / (ref_pos[k + 1] - ref_pos[k]), p and n the linear interpolations of the polyline
    vertices and of the host's vertex normals.  Returns (x, y, valid) -- valid iff ref_pos[0] <= s <= ref_pos[M - 1]."""
    L = np.longdouble
    pos64 = np.asarray(cs.ref_pos, dtype=np.float64)
    pos, P, nv = pos64.astype(L), np.asarray(cs.reference).astype(L), np.asarray(cs.normals).astype(L)
    s64, d = np.asarray(s, dtype=np.float64), np.asarray(d, dtype=np.float64).astype(L)
    valid = (s64 >= pos64[0]) & (s64 <= pos64[-1])
    k = np.clip(np.searchsorted(pos64, s64, side="right") - 1, 0, len(pos64) - 2)
    lam = (s64.astype(L) - pos[k]) / (pos[k + 1] - pos[k])
    px = P[k, 0] + lam * (P[k + 1, 0] - P[k, 0])
    py = P[k, 1] + lam * (P[k + 1, 1] - P[k, 1])
    nx = nv[k, 0] + lam * (nv[k + 1, 0] - nv[k, 0])
    ny = nv[k, 1] + lam * (nv[k + 1, 1] - nv[k, 1])
    if cs.pseudo_normal:
        return px + d * nx, py + d * ny, valid
    nn = np.sqrt(nx * nx + ny * ny)
    return px + d * (nx / nn), py + d * (ny / nn), valid


def oracle_xy_error_ulps(scene: str, frame: str):
    """(worst |oracle (x, y) - extended-precision projection of the oracle's own (s, d)| over the stored candidates' steps inside the
    projection domain, in units of np.spacing(max |coordinate| of those steps); that maximum)"""
    inp, out = oracle_step(scene, frame)
    pl = out["planes"][stored(inp, out)]
    x, y, s, d = pl[:, 0], pl[:, 1], pl[:, 7], pl[:, 8]
    ex, ey, valid = project_extended(inp.coordinate_system, s, d)
    inside = valid & ((x != 0.0) | (y != 0.0))
    top = float(max(np.abs(x[inside]).max(), np.abs(y[inside]).max()))
    err = np.maximum(np.abs(x.astype(np.longdouble) - ex), np.abs(y.astype(np.longdouble) - ey))[inside]
    return float(err.max() / np.spacing(top)), top


_XY_N = {}


def xy_ulps_allowed(frame: str) -> int:
    """n of xy_tol = 1e-9 + n spacing(max |coordinate|): twice the oracle's own worst (x, y) error of the frame over the five
    scenes, rounded up to whole units -- device and oracle each round the same operands independently"""
    if frame not in _XY_N:
        _XY_N[frame] = 2 * int(np.ceil(max(oracle_xy_error_ulps(sc, frame)[0] for sc in SCENES)))
    return _XY_N[frame]


def xy_tol(frame: str, top: float) -> float:
    return 1e-9 + xy_ulps_allowed(frame) * float(np.spacing(top))
