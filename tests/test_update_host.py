"""What the in-place step update (fx_update_state) may leave behind, audited on the host -- no GPU.

A plan step takes the update path when the resident upload has the structure of the new inputs (PlanInputs.structure_key); the
update then rewrites what FxStateUpdate carries and nothing else.  So every field of FxProblem (and of FxVehicle inside it) must be

  * carried by FxStateUpdate: the engine's own update (FrenetEngine._state_update_of) carries the new value, and the key does not
    move with it; or
  * covered by the structure key: changing the input changes that field of the problem AND the key, so such a step is uploaded; or
  * a named exception with its reason: derived from fields of the other two classes, checked here where that can be checked.

A field added to FxProblem later without a class fails `test_every_problem_field_has_exactly_one_class`: a planner whose state update
silently keeps the old value of a new input is the failure this audit exists for.
"""
import ctypes as C
import dataclasses

import numpy as np

from frenetix_motion_planner_amd import _abi, synthetic
from frenetix_motion_planner_amd.coordinate_system import CoordinateSystem
from frenetix_motion_planner_amd.problem import VehicleParams, pack_predictions

KW = dict(ref_kind="arc", v0=10.0, grid=(3, 5, 7), n_obstacles=2)
SHAPES = ("nT", "nV", "nD", "K", "P")   # FxStateUpdate states them so that a mismatch is refused; the key covers them


def _hulls():
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return build_obstacle_hulls


def _base(**kw):
    return synthetic.make_inputs(hull_builder=_hulls(), **dict(KW, **kw))


def _replace(inp, **kw):
    """the same inputs (same reference object) with some constructor arguments replaced"""
    new = dataclasses.replace(inp, **kw)
    new.predictions = getattr(inp, "predictions", None)
    return new


def _moved_predictions(inp):
    preds = {k: dict(p, pos_list=np.asarray(p["pos_list"]) + 0.5, cov_list=np.asarray(p["cov_list"]) * 1.3,
                     orientation_list=np.asarray(p["orientation_list"]) + 0.1) for k, p in inp.predictions.items()}
    return pack_predictions(preds, inp.n_samples, _hulls())


def _other_reference(inp):
    return CoordinateSystem(synthetic.reference_polyline("arc", 420, 0.45, 0.012))


def _segments(inp):
    return synthetic.offset_road_boundary(inp.coordinate_system, 3.5)


def _veh(**kw):
    return lambda i: _replace(i, vehicle=VehicleParams(**kw))


# ---- the classes ----
# carried by FxStateUpdate: field of FxProblem -> inputs with another value of it (same structure)
CARRIED = {
    "x0_lon": lambda i: _replace(i, x0_lon=i.x0_lon + 0.5),
    "x0_lat": lambda i: _replace(i, x0_lat=i.x0_lat + 0.1),
    "x0_orientation": lambda i: _replace(i, x0_orientation=i.x0_orientation + 0.1),
    "v_des": lambda i: _replace(i, v_des=i.v_des + 1.0),
    "low_vel_mode": lambda i: _replace(i, low_vel_mode=not i.low_vel_mode),
    "t_samp": lambda i: _replace(i, t_samp=i.t_samp - i.dt),
    "v_samp": lambda i: _replace(i, v_samp=i.v_samp + 0.3),
    "d_samp": lambda i: _replace(i, d_samp=i.d_samp * 0.9),
    "obs_pos": lambda i: _replace(i, obstacles=_moved_predictions(i)),
    "obs_cov_inv": lambda i: _replace(i, obstacles=_moved_predictions(i)),
    "obs_npred": lambda i: _replace(i, obstacles=dict(_moved_predictions(i), npred=np.array([7, 3], np.int32))),
    "obs_hull": lambda i: _replace(i, obstacles=_moved_predictions(i)),
    "obs_nhull": lambda i: _replace(i, obstacles=dict(_moved_predictions(i), nhull=np.array([5, 2], np.int32))),
}
# covered by the structure key: field -> inputs that differ in it
KEYED = {
    "N": lambda i: _replace(i, N=20), "dt": lambda i: _replace(i, dt=0.2),
    "mode": None,     # every bit on its own, below
    "lon_mode": lambda i: _replace(i, stop_point=True),
    "nT": lambda i: _replace(i, t_samp=np.append(i.t_samp, 2.95)), "nV": lambda i: _replace(i, v_samp=np.append(i.v_samp, 13.0)),
    "nD": lambda i: _replace(i, d_samp=np.append(i.d_samp, 0.33)),
    "shard_begin": lambda i: _shard(i, 5, 50), "shard_count": lambda i: _shard(i, 0, 50),
    "M": lambda i: _replace(i, coordinate_system=_other_reference(i)),
    **{f: (lambda i: _replace(i, coordinate_system=_other_reference(i)))
       for f in ("ref_x", "ref_y", "ref_nx", "ref_ny", "ref_pos", "ref_theta", "ref_curv", "ref_curv_d")},
    "n_cost": lambda i: _replace(i, cost_weights=dict(i.cost_weights, acceleration=0.1)),
    "cost_id": lambda i: _replace(i, cost_weights={("jerk" if k == "lateral_jerk" else k): w for k, w in i.cost_weights.items()}),
    "cost_w": lambda i: _replace(i, cost_weights={k: (w * 2 if k == "lateral_jerk" else w) for k, w in i.cost_weights.items()}),
    "K": lambda i: _replace(i, obstacles=_same_reference(i, n_obstacles=3).obstacles),
    "P": lambda i: _replace(i, obstacles=_same_reference(i, n_pred=12).obstacles),
    "n_dto": lambda i: _replace(i, dto_pos=np.array([[30.0, 1.0]])), "dto_pos": lambda i: _replace(i, dto_pos=np.array([[30.0, 1.0]])),
    **{f: (lambda i: _replace(i, road_boundary=_segments(i))) for f in ("n_bound", "bound_piece", "bound_bin", "bound_item", "bound_d_reach")},
    **{f: (lambda i: _replace(i, lanelets=synthetic.lanes_along(i.coordinate_system)))
       for f in ("n_lane", "lane_bbox", "lane_poly_off", "lane_poly", "lane_ctr_off", "lane_ctr")},
}
MODE_BITS = {   # every bit of FxProblem.mode -> inputs with that bit flipped
    "FX_MODE_DRAW_TRAJ_SET": lambda i: _replace(i, draw_traj_set=True), "FX_MODE_KINEMATIC_DEBUG": lambda i: _replace(i, kinematic_debug=True),
    "FX_MODE_WRITE_BUNDLE": lambda i: _replace(i, write_bundle=False), "FX_MODE_WRITE_COSTMAP": lambda i: _replace(i, write_costmap=False),
    "FX_MODE_COLLISION": lambda i: _replace(i, collision=False), "FX_MODE_ROAD_BOUNDARY": lambda i: _replace(i, road_boundary=_segments(i)),
    "FX_MODE_PROJ_PSEUDO_NORMAL": lambda i: _replace(i, coordinate_system=CoordinateSystem(np.asarray(i.coordinate_system.reference), pseudo_normal=True)),
}
VEHICLE_KEYED = {"a_max": _veh(a_max=9.0), "v_switch": _veh(v_switch=6.0), "delta_max": _veh(delta_max=0.9), "wheelbase": _veh(wheelbase=2.7),
                 "length": _veh(length=4.9), "width": _veh(width=1.8), "wb_rear_axle": _veh(wb_rear_axle=1.3)}
# named exceptions: field -> why neither class is needed
EXCEPTIONS = {
    "veh": "a struct: its fields are audited one by one (VEHICLE_KEYED, VEHICLE_EXCEPTIONS)",
    "tpow": "the powers of the sample times: a function of N and dt, both in the key",
    "simpson_corr": "Simpson's end correction: a function of dt, which is in the key",
    "sampling_matrix": "inputs with a sampling matrix never take the update path (FrenetEngine.plan_step_packaged, plan_batch); fx_update_state refuses "
                       "sampling values for such an upload",
    "n_rows": "the row count of the sampling matrix: see sampling_matrix",
}
VEHICLE_EXCEPTIONS = {"kappa_max": "tan(delta_max) / wheelbase, both in the key"}


def _shard(inp, begin, count):
    new = _replace(inp)
    new.shard = (begin, count)
    return new


def _same_reference(inp, **kw):
    other = _base(**kw)
    assert np.array_equal(other.coordinate_system.reference, inp.coordinate_system.reference)
    return other


def _value(struct, name):
    """a comparable form of one field of a ctypes struct: numbers as they are, arrays as tuples, pointers as addresses"""
    v = getattr(struct, name)
    if isinstance(v, C.Array):
        return tuple(v)
    if isinstance(v, C.Structure):
        return tuple(_value(v, n) for n, _ in v._fields_)
    if isinstance(v, C._Pointer):
        return C.cast(v, C.c_void_p).value
    return v


def test_every_problem_field_has_exactly_one_class():
    fields = [n for n, _ in _abi.FxProblem._fields_]
    update = [n for n, _ in _abi.FxStateUpdate._fields_]
    assert len(set(fields)) == len(fields)
    classes = (set(CARRIED), set(KEYED), set(EXCEPTIONS))
    for a in range(3):
        for b in range(a + 1, 3):
            assert not classes[a] & classes[b], classes[a] & classes[b]
    unclassed = [f for f in fields if not any(f in c for c in classes)]
    assert not unclassed, f"FxProblem fields without a class (carried by FxStateUpdate / in the structure key / named exception): {unclassed}"
    stale = set().union(*classes) - set(fields)
    assert not stale, f"classes name fields FxProblem does not have: {sorted(stale)}"
    # what the update struct carries is exactly the first class, plus the shapes it states, which the key covers
    assert set(update) == set(CARRIED) | set(SHAPES), set(update) ^ (set(CARRIED) | set(SHAPES))
    assert all(s in KEYED for s in SHAPES)
    vfields = [n for n, _ in _abi.FxVehicle._fields_]
    assert sorted(vfields) == sorted(list(VEHICLE_KEYED) + list(VEHICLE_EXCEPTIONS)), vfields
    assert all(len(r) > 20 for r in list(EXCEPTIONS.values()) + list(VEHICLE_EXCEPTIONS.values()))   # (a reason, not a placeholder)
    assert {getattr(_abi, b) for b in MODE_BITS} == {1 << k for k in range(len(MODE_BITS))}
    assert [n for n in dir(_abi) if n.startswith("FX_MODE_")] == sorted(MODE_BITS)


def test_carried_fields_reach_the_update_and_leave_the_key_alone():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    base = _base()
    key, p0, u0 = base.structure_key(), base.as_struct(), FrenetEngine._state_update_of(base)
    for f, change in CARRIED.items():
        new = change(base)
        assert new.structure_key() == key, f"{f}: the structure key moves with a field the update carries"
        assert _value(new.as_struct(), f) != _value(p0, f), f"{f}: the changed inputs do not change it"
        u = FrenetEngine._state_update_of(new)
        assert _value(u, f) != _value(u0, f), f"{f}: the engine's state update does not carry the new value"
        # ... and it carries what the problem of a fresh upload would hold
        got, want = _value(u, f), _value(new.as_struct(), f)
        if f in ("x0_lon", "x0_lat"):
            got = tuple((C.c_double * 3).from_address(got))
        assert got == (int(want) if f == "low_vel_mode" else want), f


def test_keyed_fields_change_the_structure_key():
    base = _base()
    key, p0 = base.structure_key(), base.as_struct()
    for f, change in KEYED.items():
        if change is None:
            continue
        new = change(base)
        assert _value(new.as_struct(), f) != _value(p0, f), f"{f}: the changed inputs do not change it"
        assert new.structure_key() != key, f"{f} changed and the structure key did not: the step would take the update path and keep the old value"
    for bit, change in MODE_BITS.items():
        new = change(base)
        assert (new.as_struct().mode ^ p0.mode) & getattr(_abi, bit), bit
        assert new.structure_key() != key, f"mode bit {bit} flipped and the structure key did not move"
    for f, change in VEHICLE_KEYED.items():
        new = change(base)
        assert getattr(new.as_struct().veh, f) != getattr(p0.veh, f), f
        assert new.structure_key() != key, f"vehicle.{f} changed and the structure key did not move"
    # the reference itself: the same polyline as a NEW object is another structure (the key holds the object's identity)
    again = _replace(base, coordinate_system=CoordinateSystem(np.asarray(base.coordinate_system.reference)))
    assert again.structure_key() != key


def test_the_exceptions_are_what_they_are_said_to_be():
    base = _base()
    p0 = base.as_struct()
    assert p0.veh.kappa_max == np.tan(p0.veh.delta_max) / p0.veh.wheelbase
    for change in (VEHICLE_KEYED["delta_max"], VEHICLE_KEYED["wheelbase"]):
        p = change(base).as_struct()
        assert p.veh.kappa_max == np.tan(p.veh.delta_max) / p.veh.wheelbase != p0.veh.kappa_max
    # tpow / simpson_corr: equal (N, dt) give the same table, another dt or N another one
    same = _replace(base, v_des=1.0).as_struct()
    assert _value(same, "tpow") == _value(p0, "tpow") and _value(same, "simpson_corr") == _value(p0, "simpson_corr")
    assert _value(KEYED["dt"](base).as_struct(), "simpson_corr") != _value(p0, "simpson_corr")
    assert _value(KEYED["N"](base).as_struct(), "tpow") != _value(p0, "tpow")
    # a sampling matrix keeps the inputs off the update path whatever its key says
    import inspect
    from frenetix_motion_planner_amd.engine import FrenetEngine
    m = _base(as_matrix=True)
    assert m.as_struct().n_rows == m.n_candidates and not m.as_struct().nT
    assert "sampling_matrix is None" in inspect.getsource(FrenetEngine.plan_step_packaged)
    assert "if inp.sampling_matrix is None else None" in inspect.getsource(FrenetEngine.plan_batch)


def test_state_update_through_the_extension_equals_the_long_way(monkeypatch):
    """FrenetEngine._state_update_of fills the struct in C (_fxhost.state_update) where the extension is built, field by field in Python
    otherwise: the two must agree in every field -- with hulls, without hulls, without obstacles"""
    from frenetix_motion_planner_amd import engine
    assert engine._fxhost(), "the extension _fxhost is not built"
    cases = [_base(), _base(n_obstacles=0), synthetic.make_inputs(hull_builder=None, **KW), _base(v0=1.0), CARRIED["obs_npred"](_base())]
    assert cases[2].obstacles["K"] == 2 and not cases[2].obstacles["hull"].any() and cases[3].low_vel_mode
    fast = [engine.FrenetEngine._state_update_of(c) for c in cases]
    monkeypatch.setattr(engine, "_fxhost", lambda: False)
    slow = [engine.FrenetEngine._state_update_of(c) for c in cases]
    for n, (a, b, c) in enumerate(zip(fast, slow, cases)):
        for f, _ in _abi.FxStateUpdate._fields_:
            assert _value(a, f) == _value(b, f), (n, f, _value(a, f), _value(b, f))
        assert a.K == c.obstacles["K"] and a.nT == len(c.t_samp) and (a.obs_pos is None) == (c.obstacles["K"] == 0)
        assert a.x0_lon == c.x0_lon.ctypes.data and a.low_vel_mode == int(c.low_vel_mode)
