"""Result types of a plan step -- the attribute surface of the reference's trajectory objects, backed by the
engine's structure-of-arrays TrajectoryBundle in HBM.

Reference types mirrored (read/written by planner.py:371-437, reactive_planner_cpp.py:355-357,456,470-482,
logging_helpers.py, visualization.py):
  frenetix_motion_planner/trajectories.py:56-197   CartesianSample   x, y, theta, v, a, kappa, kappa_dot
  frenetix_motion_planner/trajectories.py:200-334  CurviLinearSample s, d, theta, s_dot, s_ddot, d_dot, d_ddot
  frenetix_motion_planner/trajectories.py:337-477  TrajectorySample  + the frenetix.TrajectorySample extras
  frenetix_motion_planner/trajectories.py:480-602  TrajectoryBundle

A TrajectorySample here is a *view*: the flag word and total cost come from the arrays the engine always
reads back; the 14 planes, the per-name cost map and the polynomial coefficients of a candidate are gathered
from device memory on first access and then cached, so the object stays valid after the next plan step
overwrites the device buffers (the reference keeps `optimal_trajectory` alive across steps,
reactive_planner_cpp.py:430,437 / frenet_interface.py:277).

Samples a caller still holds when the next evaluation is about to overwrite the device buffers are *rescued*: the step reads
what they have not fetched yet in ONE batched call (engine.candidates) into a host snapshot and answers them from it from
then on (PlanStepResult.rescue, StepRegistry).
"""
import weakref
from typing import List, Optional

import numpy as np

from . import _abi

_FEAS_KEYS = {  # frenetix feasabilityMap keys (reactive_planner_cpp.py:470-482) -> reason bit
    "Curvature Constraint": 5, "Yaw rate Constraint": 6, "Curvature Rate Constraint": 7, "Acceleration Constraint": 8,
}


class _Sample:
    def __init__(self, current_time_step: int):
        self.current_time_step = current_time_step

    def length(self) -> int:
        return self.current_time_step


class CartesianSample(_Sample):
    def __init__(self, x, y, theta, v, a, kappa, kappa_dot, current_time_step):
        super().__init__(current_time_step)
        self.x, self.y, self.theta, self.v, self.a, self.kappa, self.kappa_dot = x, y, theta, v, a, kappa, kappa_dot

    def length(self) -> int:
        return len(self.x)


class CurviLinearSample(_Sample):
    def __init__(self, s, d, theta, dd=None, ddd=None, ss=None, sss=None, current_time_step=0):
        super().__init__(current_time_step)
        self.s, self.d, self.theta = s, d, theta
        self.d_dot, self.d_ddot, self.s_dot, self.s_ddot = dd, ddd, ss, sss

    def length(self) -> int:
        return len(self.s)


class PolynomialView:
    """coeffs / delta_tau of polynomial_trajectory.py:17-272 (read-only)."""

    def __init__(self, coeffs: np.ndarray, delta_tau: float):
        self.coeffs = coeffs
        self.delta_tau = delta_tau
        self.tau_0 = 0

    def squared_jerk_integral(self, t):
        c = self.coeffs
        t2 = t * t
        t3 = t2 * t
        t4 = t3 * t
        t5 = t4 * t
        return (36 * c[3] * c[3] * t + 144 * c[3] * c[4] * t2 + 240 * c[3] * c[5] * t3 + 192 * c[4] * c[4] * t3 +
                720 * c[4] * c[5] * t4 + 720 * c[5] * c[5] * t5)


class TrajectorySample:
    # what a fresh sample has not got yet lives on the class: the reference's C++ adapter asks for EVERY evaluated trajectory as
    # an object each plan step (reactive_planner_cpp.py:353-358), so a sample is a handful of instance attributes
    _planes = _costmap = _coeffs = _pkg = _sp = None
    _materialised = False
    # writable from Python (planner.py:325-326,381-382)
    _ego_risk = _obst_risk = _boundary_harm = None
    harm_occ_module = None
    # A sample is a view the step holds WEAKLY (PlanStepResult._samples), so step.sample(g) may hand out a new object for a
    # candidate whose earlier object nobody kept.  What anybody WROTE to a sample -- the planner's host walk (boundary_harm,
    # _coll_detected), an occlusion module (cost, valid, harm_occ_module), the risk fields -- therefore lives with the step
    # (PlanStepResult._written) and every object of that candidate starts from it: the state is the candidate's, not the view's.
    # Everything that is assigned from outside is kept, except the view's own caches and the two properties that store under
    # another name.
    _UNKEPT = frozenset(("_planes", "_costmap", "_coeffs", "_pkg", "_sp", "_materialised", "cost", "boundary_harm", "__dict__"))

    def __setattr__(self, name, value):
        object.__setattr__(self, name, value)
        if name not in self._UNKEPT:
            step = self._step
            w = step._written
            if w is None:
                w = step._written = {}
            w.setdefault(self.uniqueId, {})[name] = value

    @classmethod
    def bulk(cls, step: "PlanStepResult", ids) -> list:
        """the samples of `ids` (indices within the shard) from the step's cost / flag arrays, without per-sample array look-ups"""
        ids = [int(g) for g in ids]
        base = step.inputs.shard_begin
        fl, co = step.flags[ids].tolist(), step.cost[ids].tolist()
        FEAS, VALID, COLL, SEL = _abi.FX_FLAG_FEASIBLE, _abi.FX_FLAG_VALID, _abi.FX_FLAG_COLLISION, _abi.FX_FLAG_SELECTABLE
        pkg_index = step.package.index if step.package is not None else None
        out = []
        new = object.__new__
        for g, f, c in zip(ids, fl, co):
            if pkg_index is not None and g + base == pkg_index:   # the packaged winner takes the long way (it carries its arrays)
                out.append(cls(step, g))
                continue
            t = new(cls)
            t.__dict__.update(_step=step, uniqueId=g, global_id=g + base, _flags=f, _cost=c, feasible=bool(f & FEAS),
                              valid=bool(f & VALID), _coll_detected=bool(f & COLL) if (f & SEL) else None)
            out.append(t)
        return out

    @property
    def dt(self) -> float:
        return self._step.inputs.dt

    @property
    def horizon(self) -> float:
        return self._step.inputs.N * self._step.inputs.dt

    def __init__(self, step: "PlanStepResult", index: int):
        d = self.__dict__   # (the view's own fields are not "written from outside": they bypass __setattr__)
        d["_step"] = step
        d["uniqueId"] = int(index)           # index within the evaluated shard (== creation order when nothing is sharded)
        d["global_id"] = int(index) + step.inputs.shard_begin   # creation order in the whole grid (reactive_planner.py:172)
        pkg = step.package
        if pkg is not None and pkg.index == int(index) + step.inputs.shard_begin:
            # the winner: the library has already delivered everything (fx_read_package), nothing is fetched
            flags, d["_cost"] = pkg.flags, pkg.cost
            d["_planes"] = pkg.planes
            d["_pkg"] = pkg   # (coefficients and the cost map are built from the package when they are asked for)
        elif step.have_arrays:
            flags = int(step.flags[index])
            d["_cost"] = float(step.cost[index])
        else:
            # the step's cost / flag arrays have not been read back: fetch this candidate whole (one synchronisation)
            rec = step.fetch_candidate(index)
            flags = int(rec["flags"])
            d["_cost"] = float(rec["cost"])
            if rec["planes"] is not None:
                d["_planes"] = rec["planes"]
                d["_coeffs"] = (rec["lon"], rec["lat"], rec["traj_len"], rec["tau_lat"])
            if rec["raw_costs"] is not None:
                names, w = step.inputs.cost_names, step.inputs.cost_weights
                d["_costmap"] = {n: (float(rec["raw_costs"][k]), float(w[n] * rec["raw_costs"][k])) for k, n in enumerate(names)}
        if step._override is not None:   # (a cost override is installed with the step's arrays loaded: only the winner gets here)
            d["_cost"] = float(step.cost[index])
        d["_flags"] = flags
        d["feasible"] = bool(flags & _abi.FX_FLAG_FEASIBLE)
        d["valid"] = bool(flags & _abi.FX_FLAG_VALID)
        d["_coll_detected"] = bool(flags & _abi.FX_FLAG_COLLISION) if (flags & _abi.FX_FLAG_SELECTABLE) else None

    # ---- cheap attributes ----
    @property
    def cost(self) -> float:
        return self._cost

    @cost.setter
    def cost(self, value):   # (an occlusion module's calc_costs adds to it before the list is sorted, trajectories.py:557-560)
        self._cost = float(value)

    @property
    def leaves_road(self) -> Optional[bool]:
        """True/False for walked candidates when the step ran the road-boundary stage, else None"""
        bound = self._step.inputs._bound   # (FX_MODE_ROAD_BOUNDARY <=> a packed boundary with pieces: PlanInputs.mode)
        if bound is None or bound["n"] <= 0 or not (self._flags & _abi.FX_FLAG_SELECTABLE):
            return None
        return bool(self._flags & _abi.FX_FLAG_BOUNDARY)

    @property
    def boundary_harm(self):
        """planner.py:369-381: logistic regression of the velocity at the first step outside the road, 0 inside."""
        if self._boundary_harm is not None or self.leaves_road is None:
            return self._boundary_harm
        if not self.leaves_road:
            return 0
        i = int(self._step.boundary_steps[self.uniqueId])
        v = float(self.cartesian.v[i])
        c = self._step.harm_coeff
        return float(1.0 / (1.0 + np.exp(-c[0] - c[1] * v)))

    @boundary_harm.setter
    def boundary_harm(self, value):
        self._boundary_harm = value

    @property
    def reasons(self) -> int:
        """bit r set <=> infeasibility reason r (reactive_planner.py:352-545)"""
        return (self._flags >> _abi.FX_REASON_SHIFT) & 0x7FF

    @property
    def feasabilityMap(self) -> dict:
        r = self.reasons
        return {k: float((r >> b) & 1) for k, b in _FEAS_KEYS.items()}

    @property
    def sampling_parameters(self) -> np.ndarray:
        if self._sp is None:
            self._sp = self._step.inputs.candidate_params(self.uniqueId + self._step.inputs.shard_begin)
        return self._sp

    # ---- lazily gathered from the device bundle ----
    def _need_planes(self):
        if self._planes is None:
            self._planes = self._step.fetch_sample(self.uniqueId)
        return self._planes

    def materialise(self):
        """Pull everything this sample can ever need off the device (call before the next plan step)."""
        if self._materialised:
            return self
        self._materialised = True
        if self._pkg is not None:   # the library's package is host memory already: nothing on the device this sample still needs
            if self.leaves_road:
                self._boundary_harm = self.boundary_harm
            return self
        self._need_planes()
        _ = self.costMap
        _ = self.trajectory_long
        if self.leaves_road:
            self._boundary_harm = self.boundary_harm
        return self

    @property
    def cartesian(self) -> CartesianSample:
        p = self._need_planes()
        return CartesianSample(p[0], p[1], p[2], p[3], p[4], p[5], p[6], current_time_step=self.actual_traj_length)

    @property
    def curvilinear(self) -> CurviLinearSample:
        p = self._need_planes()
        return CurviLinearSample(p[7], p[8], p[9], ss=p[10], sss=p[11], dd=p[12], ddd=p[13],
                                 current_time_step=self.actual_traj_length)

    @property
    def costMap(self) -> dict:
        if self._costmap is None and self._pkg is not None:
            raw = self._pkg.raw_cost_list()
            if raw is not None:
                names, w = self._step.inputs.cost_names, self._step.inputs.cost_weights
                self._costmap = self._step._override_costmap(self.uniqueId, {n: (raw[k], float(w[n] * raw[k])) for k, n in enumerate(names)})
        if self._costmap is None:
            raw = self._step.fetch_costmap_row(self.uniqueId)
            names = self._step.inputs.cost_names
            w = self._step.inputs.cost_weights
            self._costmap = self._step._override_costmap(self.uniqueId, {n: (float(raw[k]), float(w[n] * raw[k])) for k, n in enumerate(names)})
        return self._costmap

    def _need_coeffs(self):
        if self._coeffs is None:
            pkg = self._pkg
            self._coeffs = ((pkg.lon, pkg.lat, pkg.traj_len, pkg.tau_lat) if pkg is not None
                            else self._step.fetch_coeffs(self.uniqueId))
        return self._coeffs

    @property
    def trajectory_long(self) -> PolynomialView:
        lon = self._need_coeffs()[0]
        return PolynomialView(lon, float(self.sampling_parameters[1] - self.sampling_parameters[0]))

    @property
    def trajectory_lat(self) -> PolynomialView:
        # delta_tau is what the device built the quintic over: t at speed, the arc length s_lon_goal in LOW_VEL_MODE
        # (reactive_planner.py:161-171, stop-point bundle :650-659)
        co = self._need_coeffs()
        return PolynomialView(co[1], float(co[3]))

    @property
    def actual_traj_length(self) -> int:
        return int(self._need_coeffs()[2])

    def length(self) -> int:
        return self._step.inputs.n_samples

    def __repr__(self):
        return (f"TrajectorySample(uniqueId={self.uniqueId}, cost={self._cost:.6g}, feasible={self.feasible}, "
                f"valid={self.valid})")


class StandstillSample:
    """_compute_standstill_trajectory (reactive_planner.py:579-626): plain arrays of length N (not N+1)."""

    def __init__(self, horizon, dt, cartesian, curvilinear, trajectory_long, trajectory_lat, cost_names):
        self.horizon, self.dt = horizon, dt
        self.cartesian, self.curvilinear = cartesian, curvilinear
        self.trajectory_long, self.trajectory_lat = trajectory_long, trajectory_lat
        self.uniqueId = 0
        self.feasible = None
        self.valid = None
        self.cost = 0
        self.costMap = {n: (0, 0) for n in cost_names}
        self.feasabilityMap = {k: 0.0 for k in _FEAS_KEYS}
        self._ego_risk = self._obst_risk = self.boundary_harm = self._coll_detected = None
        self.actual_traj_length = None
        self.harm_occ_module = None


_STALE_MSG = "this plan step's device data has been overwritten; materialise() samples you keep"


class StepRegistry:
    """Mix-in of an engine: the plan steps whose samples read this engine's buffers, held weakly.  Every method of the engine
    that launches an evaluation into those buffers (and close()) calls `rescue_steps()` FIRST -- `if self._steps:
    self.rescue_steps()`, one truthiness test when nothing is registered.  The rescue belongs here and not with the planner: a
    batch launches first and consumes second (multiagent.AgentBatchHip.step), so a planner that rescued in its own
    invalidate() would read the NEW step's data into the OLD samples."""
    _steps = ()

    def register_step(self, step):
        if not self._steps:
            self._steps = []
        self._steps.append(weakref.ref(step))

    def rescue_steps(self):
        steps, self._steps = self._steps, ()
        for ref in steps:
            step = ref()
            if step is not None:
                step.invalidate(rescue=True)


class _RescuedColumn:
    """a per-candidate array of a stale step of which only the rescued entries exist: column[index]"""

    def __init__(self, step, values):
        self._step, self._values = step, values

    def __getitem__(self, index):
        if not isinstance(index, (int, np.integer)):
            raise RuntimeError(_STALE_MSG)   # the whole array went with the device data: one rescued candidate at a time
        return self._values[self._step._row(index)]

    def __len__(self):
        raise RuntimeError(_STALE_MSG)

    def __array__(self, *args, **kwargs):
        raise RuntimeError(_STALE_MSG)


# PlanStepResult.ranked_ids sorts on the device from this many candidates on; below, fx_read_costs plus NumPy's stable argsort is the
# faster way to the same order (the measured switch: the host wins at 6 400 candidates, the device at 13 000)
DEVICE_SORT_MIN_CANDIDATES = 13_000


class PlanStepResult:
    """Everything one evaluated plan step produced; hands out TrajectorySample views."""

    retain = True                        # rescue the samples still held when the next evaluation overwrites the buffers
    _open = False                        # a sample that still needs the device has been handed out (the engine then knows this step)
    _snap = _snap_ids = None             # rescue(): engine.candidates() of the rescued indices (ascending) and those indices
    _written = None                      # index -> {attribute: value}: what was assigned to samples from outside (TrajectorySample.__setattr__)
    _mat = _mat_ids = None               # materialise(): engine.materialise() of the listed indices (ascending) and those indices
    _override = None                     # set_cost_override(): (cost [C], raw prediction cost [C], best index within the shard or -1)
    _extras = {}                         # set_cost_extras(): name -> (raw [C], weight) of the terms evaluated beside the step
    _risk = None                         # apply_responsibility_cost(): (ego_risk [C], obst_risk [C]) of the pass

    def __init__(self, engine, inputs, result: dict, agent: int = 0):
        self.engine, self.inputs, self.result, self.agent = engine, inputs, result, agent
        self.package = None               # engine.WinnerPackage of the step's winner when the library packaged it
        self._cost = self._flags = None   # [C] arrays, read back on first use (all_traj, masks, sorted lists)
        self._stale = False
        self._samples = {}                # index -> weak reference: the step must be able to tell which samples a caller still holds
        self.harm_coeff = (-4.591, 0.185)  # log_reg.ignore_angle const / speed (configurations/harm_parameters.json)
        self._bsteps = None

    def _opened(self):
        """the first sample that is not complete on the host leaves: from now on the engine asks this step to rescue() before it
        overwrites the buffers (a closed loop that only ever takes the packaged winner never gets here)"""
        self._open = True
        reg = getattr(self.engine, "register_step", None)
        if reg is not None:
            reg(self)

    @property
    def have_arrays(self) -> bool:
        return self._cost is not None or not hasattr(self.engine, "candidate")

    def _load_arrays(self):
        if self._cost is None:
            self._check()
            self._cost, self._flags = self.engine.costs(self.agent)

    @property
    def cost(self) -> np.ndarray:
        self._load_arrays()
        return self._cost if self._override is None else self._override[0]

    # ---- a cost computed beside the step in place of the step's own ----
    def set_cost_override(self, total, prediction, best_index, extras=None):
        """Answer `cost`, TrajectorySample.cost and costMap["prediction"] from a pass that ran beside the step: total [C] the
        re-summed cost, prediction [C] the raw prediction cost it was summed with (NaN rows: candidates without a cost, which keep
        the step's values), best_index the pass's winner within the shard (-1: none).  extras (optional): name -> (raw [C],
        weight) of further terms the pass summed in, which the step does not know -- costMap[name] = (raw, weight * raw) for the
        candidates whose raw value is not NaN.  sorted_ids, ranked_ids,
        sorted_trajectories and `best` then order by `total` with the host's stable argsort over the same pools; the device sort
        reads the step's own cost plane and is not used.  Install it before samples are handed out: a sample built earlier keeps
        the cost it was built with.  None (the default) changes nothing."""
        self._load_arrays()
        total, prediction = np.asarray(total, np.float64), np.asarray(prediction, np.float64)
        if total.shape != self._cost.shape or prediction.shape != self._cost.shape:
            raise ValueError(f"cost override of {total.shape} / {prediction.shape} entries for {self._cost.shape} candidates")
        costed = (self._flags & _abi.FX_FLAG_COSTED) != 0
        self.set_cost_extras({name: (np.where(costed, np.asarray(raw, np.float64), np.nan), weight)
                              for name, (raw, weight) in (extras or {}).items()})
        self._override = (np.where(costed, total, self._cost), np.where(costed, prediction, np.nan), int(best_index))
        self._host_orders = None

    def set_cost_extras(self, extras):
        """name -> (raw [C], weight): terms evaluated beside the step, which the step does not know.  costMap[name] = (raw,
        weight * raw) for the candidates whose raw value is not NaN, and the bulk logs get a column per name.  Without
        set_cost_override the step's costs and orders stay its own: that is for a term that is 0.0 for every candidate."""
        ex = {}
        for name, (raw, weight) in extras.items():
            raw = np.asarray(raw, np.float64)
            if raw.shape != (self.inputs.n_candidates,):
                raise ValueError(f"extra term {name!r} of {raw.shape} entries for {self.inputs.n_candidates} candidates")
            ex[name] = (raw, float(weight))
        self._extras = ex

    def cost_columns(self, ids):
        """(names, raw [len(ids), n], weights [n]) of the cost terms of the candidates `ids` as costMap reports them: the step's
        cost map with the override's prediction entry, then the extra terms (0.0 where a candidate has none)."""
        names = list(self.inputs.cost_names)
        raw = np.array(self.engine.costmap(self.agent)[ids], np.float64) if names else np.zeros((len(ids), 0))
        weights = [self.inputs.cost_weights[n] for n in names]
        if self._override is not None and "prediction" in names:
            p, k = self._override[1][ids], names.index("prediction")
            raw[:, k] = np.where(np.isnan(p), raw[:, k], p)
        for name, (r, w) in self._extras.items():
            names.append(name)
            raw = np.column_stack([raw, np.nan_to_num(r[ids], nan=0.0)])
            weights.append(w)
        return names, raw, np.array(weights, np.float64)

    def apply_responsibility_cost(self, params, cost_params, weight: float, prediction: str = "step", result=None):
        """Run engine.responsibility_cost over every candidate of this step -- the obstacles and reach sets are the engine's last
        ones -- and install its result: total and best as the cost override, costMap["responsibility"], and _ego_risk /
        _obst_risk of every sample of the step (partial_cost_functions.py:373-374).  prediction "probability": the collision
        probability replaces the step's prediction entry in the same override.  result: this agent's dict of a
        responsibility_cost_batch call over the same step, installed exactly as the computed one is.  Returns the pass's dict."""
        self._check()
        r = result if result is not None else self.engine.responsibility_cost(params, cost_params, weight, agent=self.agent,
                                                                              prediction=prediction)
        pred = r["prediction"] if r["prediction"] is not None else np.full(len(r["total"]), np.nan)
        self.set_cost_override(r["total"], pred, r["best_index"], extras={"responsibility": (r["resp"], weight)})
        self._risk = (r["ego_risk"], r["obst_risk"])
        return r

    def _risk_fields(self, t):
        """_ego_risk / _obst_risk of a new sample from the responsibility pass (what was written to the candidate since wins)"""
        rk = self._risk
        if rk is not None and not np.isnan(rk[0][t.uniqueId]):
            t.__dict__["_ego_risk"], t.__dict__["_obst_risk"] = float(rk[0][t.uniqueId]), float(rk[1][t.uniqueId])

    def apply_prediction_probability(self, ego_length: float, ego_width: float, result=None):
        """Run engine.prediction_probability over every candidate of this step -- the obstacles are the ones of the engine's last
        set_risk_obstacles -- and install its result as the cost override.  result: this agent's dict of a
        prediction_probability_batch call over the same step, installed exactly as the computed one is.  Returns the pass's dict."""
        self._check()
        r = result if result is not None else self.engine.prediction_probability(ego_length, ego_width, agent=self.agent)
        self.set_cost_override(r["total"], r["prob"], r["best_index"])
        return r

    def _override_costmap(self, index, costmap: dict) -> dict:
        ov = self._override
        if ov is not None and "prediction" in costmap and not np.isnan(ov[1][index]):
            p = float(ov[1][index])
            costmap["prediction"] = (p, float(self.inputs.cost_weights["prediction"] * p))
        for name, (raw, weight) in self._extras.items():
            if not np.isnan(raw[index]):
                costmap[name] = (float(raw[index]), float(weight * raw[index]))
        return costmap

    @property
    def flags(self) -> np.ndarray:
        self._load_arrays()
        return self._flags

    # ---- listed candidates of a step that stored no bundle ----
    def materialise(self, ids):
        """Install the rows of the candidates `ids` (indices within the shard) of a step that ran without the bundle or the cost
        map: engine.materialise re-walks them on the device and the host keeps its rows, from which sample(g), fetch_sample,
        fetch_coeffs, fetch_costmap_row and fetch_candidate answer the listed candidates -- now and after the next evaluation;
        unlisted candidates raise what they raise on such a step.  A later call adds to the set.  A step that stored everything
        needs none of this and keeps answering from its own arrays."""
        self._check()
        if self.inputs.write_bundle and self.inputs.write_costmap:
            return
        ids = np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))
        if self._mat_ids is not None:
            ids = np.union1d(self._mat_ids, ids)
        self._mat = self.engine.materialise(ids, self.agent)
        self._mat_ids = ids

    def install_materialised(self, ids, rows):
        """the rows of `ids` (ascending, without duplicates) as a call outside made them for this step's agent
        (engine.materialise_batch): what materialise(ids) would have installed"""
        self._check()
        self._mat = rows
        self._mat_ids = np.asarray(ids, dtype=np.int64).reshape(-1)

    def _mat_row(self, index):
        """row of candidate `index` among the materialised ones, None when it is not listed"""
        ids = self._mat_ids
        if ids is not None:
            k = int(np.searchsorted(ids, index))
            if k < len(ids) and ids[k] == index:
                return k
        return None

    def fetch_candidate(self, index) -> dict:
        k = self._mat_row(index)
        if k is not None:
            return {name: self._mat[name][k] for name in ("planes", "lon", "lat", "tau_lat", "traj_len", "raw_costs", "cost", "flags")}
        if self._stale:
            k, sn = self._row(index), self._snap
            one = lambda name: None if sn[name] is None else sn[name][k]
            return dict(planes=one("planes"), lon=one("lon"), lat=one("lat"), tau_lat=one("tau_lat"), traj_len=one("traj_len"),
                        raw_costs=one("raw_costs"), cost=sn["cost"][k], flags=sn["flags"][k])
        return self.engine.candidate(int(index), self.agent)

    @property
    def boundary_steps(self):
        """[C] first step outside the road per candidate; of a stale step only the rescued entries exist: index it with one
        candidate (anything else raises the stale-step error)"""
        if self._bsteps is None:
            if self._stale and self._snap is not None and self._snap["boundary_step"] is not None:
                return _RescuedColumn(self, self._snap["boundary_step"])
            self._check()
            self._bsteps = self.engine.boundary_steps(self.agent)
        return self._bsteps

    # ---- life beyond the next evaluation ----
    def live_samples(self) -> list:
        """the samples handed out that somebody still references"""
        return [t for t in (ref() for ref in self._samples.values()) if t is not None]

    def rescue(self):
        """The engine is about to overwrite this step's device data: read what the samples still held have not fetched yet --
        ONE engine.candidates() call -- into a host snapshot; fetch_* answer the rescued indices from it once the step is
        stale.  Samples that are complete (materialised, or carrying the winner package) need nothing.  A no-op on a stale
        step; on a fresh one a later call replaces the snapshot by one of the samples held THEN."""
        if self._stale or not self._open:
            return
        ids = set()
        for ref in self._samples.values():
            t = ref()
            if t is not None and not t._materialised and t._pkg is None and self._mat_row(t.uniqueId) is None:
                ids.add(t.uniqueId)   # (a materialised candidate's rows are on the host already)
        if not ids:
            return
        ids = np.array(sorted(ids), dtype=np.int64)
        eng = self.engine
        self._snap = eng.candidates(ids, self.agent) if hasattr(eng, "candidates") else self._read_per_sample(ids)
        self._snap_ids = ids

    def _read_per_sample(self, ids) -> dict:
        """what engine.candidates(ids) returns, from the per-sample methods of an engine without it (duck-typed stand-ins)"""
        eng, inp, a = self.engine, self.inputs, self.agent
        planes = lon = lat = tau = tl = raw = bst = None
        if inp.write_bundle:
            planes = np.stack([eng.sample(int(g), a) for g in ids])
            co = [eng.coeffs(int(g), a) for g in ids]
            lon, lat = np.stack([c[0] for c in co]), np.stack([c[1] for c in co])
            tl, tau = np.array([c[2] for c in co], np.int32), np.array([c[3] for c in co])
        if inp.write_costmap and len(inp.cost_names) > 0:
            if not hasattr(self, "_cm"):
                self._cm = eng.costmap(a)
            raw = self._cm[ids]
        if inp._bound is not None and inp._bound["n"] > 0:
            bst = self.boundary_steps[ids]
        return dict(planes=planes, lon=lon, lat=lat, tau_lat=tau, traj_len=tl, raw_costs=raw, cost=self.cost[ids].copy(),
                    flags=self.flags[ids].copy(), boundary_step=bst)

    def invalidate(self, rescue: bool = False):
        """This step's device data is gone -- rescue=False: already overwritten (the meaning this call always had); rescue=True:
        ABOUT to be overwritten, the caller runs before the launch, so what is still held is read first (unless `retain` is off)."""
        if self._stale:
            return
        if rescue and self._open and self.retain:
            self.rescue()
        self._stale = True

    def _check(self):
        if self._stale:
            raise RuntimeError(_STALE_MSG)

    def _row(self, index) -> int:
        """row of candidate `index` in the snapshot of a stale step; the stale-step error for an index that was not rescued"""
        ids = self._snap_ids
        if ids is not None:
            k = int(np.searchsorted(ids, index))
            if k < len(ids) and ids[k] == index:
                return k
        raise RuntimeError(_STALE_MSG)

    def _rescued(self, name, index, missing):
        part = self._snap[name] if self._snap is not None else None
        k = self._row(index)
        if part is None:   # the step did not produce it: what the library answers on a fresh step
            raise ValueError(f"fxplan: plan step ran without {missing} (status {_abi.FX_ERR_NOT_READY})")
        return part, k

    def fetch_sample(self, index):
        k = self._mat_row(index)
        if k is not None:
            return self._mat["planes"][k]
        if self._stale:
            part, k = self._rescued("planes", index, "FX_MODE_WRITE_BUNDLE")
            return part[k]
        return self.engine.sample(index, self.agent)

    def fetch_costmap_row(self, index):
        k = self._mat_row(index)
        if k is not None:
            return self._mat["raw_costs"][k]
        if self._stale:
            part, k = self._rescued("raw_costs", index, "FX_MODE_WRITE_COSTMAP")
            return part[k]
        if not hasattr(self, "_cm"):
            self._cm = self.engine.costmap(self.agent)
        return self._cm[index]

    def fetch_coeffs(self, index):
        k = self._mat_row(index)
        if k is not None:
            sn = self._mat
            return sn["lon"][k], sn["lat"][k], int(sn["traj_len"][k]), float(sn["tau_lat"][k])
        if self._stale:
            lon, k = self._rescued("lon", index, "FX_MODE_WRITE_BUNDLE")
            sn = self._snap
            return lon[k], sn["lat"][k], int(sn["traj_len"][k]), float(sn["tau_lat"][k])
        return self.engine.coeffs(index, self.agent)

    def sample(self, index: int) -> TrajectorySample:
        ref = self._samples.get(index)
        t = ref() if ref is not None else None
        if t is None:
            t = TrajectorySample(self, index)
            self._samples[index] = weakref.ref(t)
            if t._pkg is None and not self._open:
                self._opened()
            self._risk_fields(t)
            w = self._written
            if w is not None and index in w:   # an earlier object of this candidate was written to and dropped
                t.__dict__.update(w[index])
        return t

    # ---- views the planner needs ----
    @property
    def n_candidates(self) -> int:
        return int(self.result["n_candidates"])

    def mask(self, bit) -> np.ndarray:
        return (self.flags & bit) != 0

    def sorted_ids(self, pool_bit=_abi.FX_FLAG_COSTED) -> np.ndarray:
        """ids of the pool in stable cost order (TrajectoryBundle.sort, trajectories.py:524-561)."""
        ids = np.nonzero(self.mask(pool_bit))[0]
        return ids[np.argsort(self.cost[ids], kind="stable")]

    # ---- the order by rank, sorted on the device ----
    _rank_pool = None                    # (require, exclude, engine.sort_serials[agent]) of the device order this step last asked for
    _rank_counts = (0, 0)
    _host_orders = None                  # (require, exclude) -> ids by rank, where the host arrays answered

    def _device_order(self, require, exclude):
        """(n_pool, n_nan) with the engine's device order of this step being that of the pool, sorting when it is not; None when
        the host arrays answer: a stale step, an engine without `ranked`, or an agent below DEVICE_SORT_MIN_CANDIDATES (the
        measured size under which the host's NumPy sort is the faster one)"""
        eng = self.engine
        if self._stale or not hasattr(eng, "ranked") or self.n_candidates < DEVICE_SORT_MIN_CANDIDATES or self._override is not None:
            return None   # (an override: the device sort reads the step's own cost plane)
        serials = getattr(eng, "sort_serials", None) or {}   # (there is one order per agent on the device: another agent's sort leaves it)
        if self._rank_pool != (require, exclude, serials.get(self.agent, 0)):
            self._rank_counts = eng.sort_candidates(self.agent, require, exclude)
            self._rank_pool = (require, exclude, (getattr(eng, "sort_serials", None) or {}).get(self.agent, 0))
        return self._rank_counts

    def _host_order(self, require, exclude):
        if self._host_orders is None:
            self._host_orders = {}
        order = self._host_orders.get((require, exclude))
        if order is None:
            ids = np.nonzero(((self.flags & require) == require) & ((self.flags & exclude) == 0))[0]
            order = self._host_orders[(require, exclude)] = ids[np.argsort(self.cost[ids], kind="stable")]
        return order

    def ranked_count(self, pool_bit=_abi.FX_FLAG_COSTED, exclude=0):
        """(n_pool, n_nan) of the pool (flags & pool_bit) == pool_bit and (flags & exclude) == 0: its size and how many of its
        members have a NaN cost -- they are the last n_nan ranks"""
        counts = self._device_order(int(pool_bit), int(exclude))
        if counts is None:
            ids = self._host_order(int(pool_bit), int(exclude))
            counts = (len(ids), int(np.isnan(self.cost[ids]).sum()))
        return counts

    def ranked_ids(self, first, n, pool_bit=_abi.FX_FLAG_COSTED, exclude=0) -> np.ndarray:
        """ids [first, first + n) of the pool in stable cost order, clipped to the pool like a slice: sorted_ids(pool_bit)[first:first + n]
        -- from DEVICE_SORT_MIN_CANDIDATES candidates on without reading the C costs: the device sorts once per (step, pool), ranges
        are read by rank; below it the host reads the costs once per step and sorts once per pool.  A stale or rescued step
        answers from its host arrays, as sorted_ids does."""
        first, n = max(int(first), 0), max(int(n), 0)
        counts = self._device_order(int(pool_bit), int(exclude))
        if counts is None:
            return self._host_order(int(pool_bit), int(exclude))[first:first + n]
        n = min(n, max(counts[0] - first, 0))
        return self.engine.ranked(first, n, self.agent) if n > 0 else np.empty(0, np.int64)

    def samples(self, ids) -> List[TrajectorySample]:
        """the samples of `ids` (indices within the shard), in that order"""
        ids = [int(g) for g in ids]
        known = self._samples
        todo = [g for g in ids if g not in known or known[g]() is None]
        made = {}
        if len(todo) > 8:   # many new samples at once (the adapter's sorted list): built from the arrays in one go
            if not self._open:
                self._opened()
            w = self._written
            for t in TrajectorySample.bulk(self, todo):
                known[t.uniqueId] = weakref.ref(t)
                made[t.uniqueId] = t
                self._risk_fields(t)
                if w is not None and t.uniqueId in w:
                    t.__dict__.update(w[t.uniqueId])
        return [made.get(g) or self.sample(g) for g in ids]

    def sorted_trajectories(self, pool_bit=_abi.FX_FLAG_COSTED, limit: Optional[int] = None) -> List[TrajectorySample]:
        ids = self.sorted_ids(pool_bit)
        if limit is not None:
            ids = ids[:limit]
        return self.samples(ids)

    @property
    def best(self) -> Optional[TrajectorySample]:
        if self._override is not None:
            g = self._override[2]
            return self.sample(g) if g >= 0 else None
        g = self.result["best_index"] - self.inputs.shard_begin
        return self.sample(int(g)) if self.result["best_index"] >= 0 else None
