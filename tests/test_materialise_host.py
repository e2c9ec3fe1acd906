"""Host side of the materialised candidates without a GPU: PlanStepResult.materialise and the planner's
sparse_bundle_k on a stand-in engine that behaves like a select-only FrenetEngine, and the three new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

from frenetix_motion_planner_amd import VehicleParams, _abi, _lib, synthetic
from frenetix_motion_planner_amd.trajectories import PlanStepResult
from tests.oracle_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fx_materialise_candidates_agent", "fx_read_materialised_agent", "fx_read_package_materialised")


class SelectOnlyOracle(OracleEngine):
    """OracleEngine that answers like the library after a step without the bundle / the cost map -- the per-candidate parts are
    refused -- and whose `materialise` runs the oracle for the listed ids, rows in the caller's order."""

    def __init__(self):
        super().__init__()
        self.materialised = []   # the lists it was asked for

    def _refuse(self, agent, what):
        inp = self.last[agent][0]
        if not getattr(inp, what):
            raise ValueError(f"fxplan: plan step ran without it (status {_abi.FX_ERR_NOT_READY})")

    def sample(self, index, agent=0):
        self._refuse(agent, "write_bundle")
        return super().sample(index, agent)

    def coeffs(self, index, agent=0):
        self._refuse(agent, "write_bundle")
        return super().coeffs(index, agent)

    def costmap(self, agent=0):
        self._refuse(agent, "write_costmap")
        return super().costmap(agent)

    def materialise(self, ids, agent=0):
        ids = np.asarray(ids, np.int64).reshape(-1)
        out = self.last[agent][1]
        if ((ids < 0) | (ids >= len(out["cost"]))).any():
            raise ValueError("fxplan: candidate out of range (status -1)")
        self.materialised.append(ids.copy())
        return dict(planes=out["planes"][ids].copy(), lon=out["coeff_lon"][ids].copy(), lat=out["coeff_lat"][ids].copy(),
                    tau_lat=out["tau_lat"][ids].copy(), traj_len=out["traj_len"][ids].astype(np.int32),
                    raw_costs=out["costmap"][ids].copy(), cost=out["cost"][ids].copy(), flags=out["flags"][ids].copy(),
                    boundary_step=None)


KW = dict(ref_kind="arc", v0=10.0, grid=(4, 6, 7), n_obstacles=3)


def _step(**kw):
    from oracle import oracle
    eng = SelectOnlyOracle()
    inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **dict(KW, **kw))
    res = eng.plan_step(inp)
    return eng, inp, PlanStepResult(eng, inp, res), eng.last[0][1]


def _costed(out, n):
    return [int(g) for g in np.nonzero(out["costed"])[0][:n]]


def test_listed_candidates_answer_in_any_order_with_duplicates():
    eng, inp, step, out = _step(write_bundle=False, write_costmap=False)
    a, b, c = _costed(out, 3)
    step.materialise([c, a, c, b, a])
    assert np.array_equal(eng.materialised[-1], sorted({a, b, c}))   # the set is ascending and de-duplicated
    for g in (b, c, a):
        t = step.sample(g)
        assert np.array_equal(t.cartesian.x, out["planes"][g][0]) and np.array_equal(t.curvilinear.d, out["planes"][g][8])
        assert t.costMap[inp.cost_names[0]][0] == out["costmap"][g][0]
        assert t.actual_traj_length == out["traj_len"][g] and t.trajectory_lat.delta_tau == out["tau_lat"][g]
        assert step.fetch_candidate(g)["cost"] == out["cost"][g]
        assert np.array_equal(step.fetch_sample(g), out["planes"][g])
        assert t.sampling_parameters.shape == (13,) and set(t.feasabilityMap)
    # a later call adds to the set
    d = _costed(out, 4)[3]
    step.materialise([d])
    assert np.array_equal(eng.materialised[-1], sorted({a, b, c, d}))
    assert np.array_equal(step.sample(a).cartesian.y, out["planes"][a][1]) and np.array_equal(step.fetch_sample(d), out["planes"][d])


def test_unlisted_candidates_raise_what_a_select_only_step_raises():
    eng, inp, step, out = _step(write_bundle=False, write_costmap=False)
    a, b = _costed(out, 2)
    step.materialise([a])
    t = step.sample(b)
    assert t.cost == out["cost"][b]   # cost and flags are the step's own
    with pytest.raises(ValueError, match="status -2"):
        t.cartesian
    with pytest.raises(ValueError, match="status -2"):
        t.costMap
    with pytest.raises(ValueError):
        step.materialise([len(out["cost"])])
    assert np.array_equal(step.sample(a).cartesian.x, out["planes"][a][0])   # the refused call left the set as it was


def test_held_samples_are_rescued_from_the_set():
    eng, inp, step, out = _step(write_bundle=False, write_costmap=False)
    a, b, c = _costed(out, 3)
    step.materialise([a, b])
    ta, tc = step.sample(a), step.sample(c)
    step.invalidate(rescue=True)     # the next evaluation is about to overwrite the device
    eng.plan_step(synthetic.make_inputs(**dict(KW, v0=6.0, write_bundle=False, write_costmap=False)))
    assert np.array_equal(ta.cartesian.x, out["planes"][a][0]) and ta.costMap[inp.cost_names[0]][0] == out["costmap"][a][0]
    assert np.array_equal(step.sample(b).curvilinear.d, out["planes"][b][8])   # listed, first asked for after the step went stale
    with pytest.raises((ValueError, RuntimeError)):
        tc.cartesian                 # unlisted: nothing to rescue it from
    with pytest.raises(RuntimeError):
        step.materialise([c])        # a stale step cannot be re-walked


def test_a_step_that_stored_everything_needs_no_set():
    eng, inp, step, out = _step()
    step.materialise([1, 2, 3])
    assert eng.materialised == [] and step._mat is None
    assert np.array_equal(step.sample(2).cartesian.x, out["planes"][2][0])


def _planner(engine, **cfg):
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig, ReactivePlannerHip, ReactivePlannerState
    rp = ReactivePlannerHip(PlannerConfig(**cfg), VehicleParams(), engine=engine)
    ref = synthetic.reference_polyline("arc", 400, 0.5, 0.01)
    cs = synthetic.CoordinateSystem(ref)
    s0 = float(cs.ref_pos[40] + 0.1)
    x0 = ReactivePlannerState(time_step=0, position=cs.convert_to_cartesian_coords(s0, 0.2), orientation=float(cs.ref_theta[40]), velocity=10.0)
    rp.update_externals(reference_path=ref, x_0=x0, desired_velocity=12.0, predictions=synthetic.synthetic_predictions(cs, 5, 30, 0.1, s0, np.random.default_rng(1)))
    return rp


def test_sparse_bundle_k_zero_builds_the_inputs_of_today():
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
    assert PlannerConfig().sparse_bundle_k == 0
    a, b = _planner(OracleEngine())._inputs_for_level(2), _planner(OracleEngine(), sparse_bundle_k=8)._inputs_for_level(2)
    assert a.write_bundle and a.write_costmap and not b.write_bundle and not b.write_costmap
    both = _abi.FX_MODE_WRITE_BUNDLE | _abi.FX_MODE_WRITE_COSTMAP
    assert a.mode & both == both and b.mode == a.mode & ~both
    for name in ("t_samp", "v_samp", "d_samp", "x0_lon", "x0_lat"):
        assert np.array_equal(getattr(a, name), getattr(b, name))
    assert a.cost_names == b.cost_names and a.n_candidates == b.n_candidates


def test_planner_with_a_sparse_set_chooses_and_packages_the_same_trajectory():
    ref, eng = _planner(OracleEngine()), SelectOnlyOracle()
    rp = _planner(eng, sparse_bundle_k=8)
    pa, pb = ref.plan(), rp.plan()
    assert pa is not None and pb is not None
    assert rp.optimal_trajectory.uniqueId == ref.optimal_trajectory.uniqueId
    assert rp.last_step.result == ref.last_step.result
    best = rp.optimal_trajectory.uniqueId
    assert best in eng.materialised[0] and 1 < len(eng.materialised[0]) <= 9   # the winner and the first 8 of the top-k
    for sa, sb in zip(pa[0], pb[0]):
        assert np.array_equal(sa.position, sb.position) and sa.orientation == sb.orientation and sa.velocity == sb.velocity
        assert sa.yaw_rate == sb.yaw_rate and sa.steering_angle == sb.steering_angle
    assert np.array_equal(np.asarray(pa[2]), np.asarray(pb[2])) and np.array_equal(np.asarray(pa[3]), np.asarray(pb[3]))
    assert set(rp.optimal_trajectory.costMap) == set(ref.optimal_trajectory.costMap)


def test_new_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    L = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", hdr), f"{sym} is not declared in fxplan.h"
        assert sym in _lib.exported_symbols() and hasattr(L, sym), sym
        assert getattr(L, sym).argtypes is not None
    assert _abi.FX_ABI_VERSION == 15 and L.fx_abi_version() == 15 and "#define FX_ABI_VERSION 15" in hdr
