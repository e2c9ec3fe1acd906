"""The `frenetix`-route handler of test_frenetix_handler_drives_the_engine (its functors, predictions and 800-row sampling matrix) as a
builder shared by the tests of the retained samples, of the batched read-back and by tools/bench_readback.py."""
import numpy as np

from frenetix_motion_planner_amd import VehicleParams, synthetic


def make_handler(engine=None):
    """the handler and functors of test_frenetix_handler_drives_the_engine; matrix(ds0, ss0) builds its 800-row matrix"""
    from frenetix_motion_planner_amd import frenetix_compat as fx
    from frenetix_motion_planner_amd.sampling import SamplingHandler, generate_sampling_matrix, v_sampling_bounds
    veh = VehicleParams()
    ref = synthetic.reference_polyline("arc", 400, 0.5, 0.01)
    cs = fx.CoordinateSystemWrapper(ref)
    h = fx.TrajectoryHandler(dt=0.1, engine=engine)
    h.add_feasability_function(fx.CheckYawRateConstraint(deltaMax=veh.delta_max, wheelbase=veh.wheelbase, wholeTrajectory=False))
    h.add_feasability_function(fx.CheckAccelerationConstraint(switchingVelocity=veh.v_switch, maxAcceleration=veh.a_max, wholeTrajectory=False))
    h.add_feasability_function(fx.CheckCurvatureConstraint(deltaMax=veh.delta_max, wheelbase=veh.wheelbase, wholeTrajectory=False))
    h.add_feasability_function(fx.CheckCurvatureRateConstraint(wheelbase=veh.wheelbase, velocityDeltaMax=veh.v_delta_max, wholeTrajectory=False))
    for cls, name, w in ((fx.CalculateLateralJerkCost, "lateral_jerk", 0.2), (fx.CalculateLongitudinalJerkCost, "longitudinal_jerk", 0.2),
                         (fx.CalculateDistanceToReferencePathCost, "distance_to_reference_path", 5.0)):
        h.add_cost_function(cls(name, w))
    h.add_function(fx.FillCoordinates(lowVelocityMode=False, initialOrientation=float(cs.ref_theta[40]), coordinateSystem=cs, horizon=3))
    h.add_cost_function(fx.CalculateVelocityOffsetCost("velocity_offset", 1.0, 12.0, 0.1, 1.1, limit_to_t_min=False, norm_order=2))
    preds = synthetic.synthetic_predictions(cs, 3, 30, 0.1, float(cs.ref_pos[40]), np.random.default_rng(2))
    pobj = {}
    for k, p in preds.items():
        path = [fx.PoseWithCovariance(np.append(p["pos_list"][j], 0.0), np.array([0, 0, np.sin(p["orientation_list"][j] / 2),
                                                                                    np.cos(p["orientation_list"][j] / 2)]),
                                      np.pad(p["cov_list"][j], ((0, 4), (0, 4)))) for j in range(30)]
        pobj[k] = fx.PredictedObject(k, path, p["shape"]["length"], p["shape"]["width"])
    h.add_cost_function(fx.CalculateCollisionProbabilityFast("prediction", 0.2, pobj, veh.length, veh.width, veh.wb_rear_axle))
    sh = SamplingHandler(dt=0.1, max_sampling_number=3, t_min=1.1, horizon=3.0, delta_d_min=-3, delta_d_max=3, d_ego_pos=False)
    sh.set_v_sampling(*v_sampling_bounds(10.0, veh.a_max, 3.0, veh.v_max))

    def matrix(ds0=0.0, ss0=10.0):
        t, v, d = sh.ordered_ranges(2, 0.2, cpp_style=True, ss0=ss0, t_full=3.0)
        m = generate_sampling_matrix(t0_range=0.0, t1_range=t, s0_range=float(cs.ref_pos[40] + 0.1) + ds0, ss0_range=ss0,
                                     sss0_range=0.0, ss1_range=v, sss1_range=0, d0_range=0.2, dd0_range=0.0, ddd0_range=0.0,
                                     d1_range=d, dd1_range=0.0, ddd1_range=0.0)
        assert m.shape == (800, 13)
        return m
    return h, matrix


def evaluate(h, m):
    h.generate_trajectories(m, False)
    h.evaluate_all_current_functions_concurrent(True)
