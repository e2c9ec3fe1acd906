"""FrenetEngine: thin object wrapper over the C-ABI (one context = one planner's device state).

Plays the role of `frenetix.TrajectoryHandler` behind reactive_planner_cpp.py:49,255-256,345-353: it takes
the shared inputs of a plan step, runs the fused HIP pipeline and hands back the winner, counters and
lazily-materialised per-candidate data.  Batched form (`plan_batch`) evaluates several agents in one launch
(the GPU analogue of AgentBatch._step_agents, agent_batch.py:186-189).
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _abi
from ._lib import check, lib
from .problem import PlanInputs, hypothesis_arrays
from .trajectories import StepRegistry


def build_obstacle_hulls(n_pred, pos, yaw, length, width) -> np.ndarray:
    """OBB-sum hulls of consecutive predicted boxes (host helper of the library)."""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    yaw = np.ascontiguousarray(yaw, dtype=np.float64)
    out = np.zeros((max(int(n_pred) - 1, 1), 6))
    n = C.c_int32(0)
    check(lib().fx_build_obstacle_hulls(int(n_pred), pos.ctypes.data_as(C.POINTER(C.c_double)),
                                        yaw.ctypes.data_as(C.POINTER(C.c_double)), float(length), float(width),
                                        out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
    return out[:n.value]


def _build_obstacle_hulls_batch(n_use, pos, yaw, length, width, hull, nhull):
    """fx_build_obstacle_hulls_batch: pos [K][P][2], yaw [K][P] -> hull [K][P-1][6], nhull [K] (in place)"""
    K, P = pos.shape[0], pos.shape[1]
    length, width = np.ascontiguousarray(length, dtype=np.float64), np.ascontiguousarray(width, dtype=np.float64)
    check(lib().fx_build_obstacle_hulls_batch(K, P, n_use.ctypes.data, pos.ctypes.data, yaw.ctypes.data, length.ctypes.data,
                                              width.ctypes.data, hull.ctypes.data, nhull.ctypes.data))


def invert_cov2(m: np.ndarray) -> np.ndarray:
    """[n, 2, 2] -> [n, 4]: np.linalg.inv of every matrix, bit for bit (fx_invert_cov2); LinAlgError for a singular one"""
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 4)
    out = np.empty_like(m)
    if lib().fx_invert_cov2(len(m), m.ctypes.data, out.ctypes.data) != 0:
        raise np.linalg.LinAlgError("Singular matrix")
    return out


def _pack_predictions_c(entries, P: int, n_samples: int):
    """fx_pack_predictions: entries = [(pos [n,2], cov [n,2,2], yaw [n] or None, length, width)] -> packed arrays"""
    K = len(entries)
    lens = [len(e[0]) for e in entries]
    i64 = C.c_int64 * K
    if all(e[2] is not None and len(e[2]) == n and len(e[1]) == n for e, n in zip(entries, lens)):
        # the usual case (every obstacle with orientations and a shape): three concatenations, the pointer columns are
        # base + offset -- one .ctypes access per kind instead of one per array
        pos_all = np.concatenate([e[0] for e in entries])
        cov_all = np.concatenate([e[1] for e in entries])
        yaw_all = np.concatenate([e[2] for e in entries])
        bp, bc, by = pos_all.ctypes.data, cov_all.ctypes.data, yaw_all.ctypes.data
        pp, pc, py, off = [], [], [], 0
        for n in lens:
            pp.append(bp + 16 * off); pc.append(bc + 32 * off); py.append(by + 8 * off)
            off += n
    else:
        pp = [e[0].ctypes.data for e in entries]
        pc = [e[1].ctypes.data for e in entries]
        py = [0 if e[2] is None else e[2].ctypes.data for e in entries]
    f64 = C.c_double * K
    sizes = (2 * K * P, 4 * K * P, 6 * K * (P - 1))
    out = np.empty(sum(sizes))   # outputs in one block, handed out as views
    cnt = np.empty((2, K), np.int32)
    o0, c0 = out.ctypes.data, cnt.ctypes.data
    rc = lib().fx_pack_predictions(K, P, int(n_samples), (C.c_int32 * K)(*lens), i64(*pp), i64(*pc), i64(*py),
                                   f64(*[e[3] for e in entries]), f64(*[e[4] for e in entries]),
                                   o0, o0 + 8 * sizes[0], c0, o0 + 8 * (sizes[0] + sizes[1]), c0 + 4 * K)
    if rc != 0:
        if b"singular" in lib().fx_last_error():
            raise np.linalg.LinAlgError("Singular matrix")
        check(rc)
    return dict(K=K, P=P, pos=out[:sizes[0]].reshape(K, P, 2), cov_inv=out[sizes[0]:sizes[0] + sizes[1]].reshape(K, P, 4),
                npred=cnt[0], hull=out[sizes[0] + sizes[1]:].reshape(K, P - 1, 6), nhull=cnt[1])


_FXHOST = None


def _fxhost():
    """the CPython extension `_fxhost` (csrc/fx_host_ext.c, built next to the package by `make`); False when it is not there"""
    global _FXHOST
    if _FXHOST is None:
        try:
            from . import _fxhost as m
            _FXHOST = (m, C.cast(lib().fx_pack_predictions, C.c_void_p).value, C.cast(lib().fx_plan_batch_packaged, C.c_void_p).value,
                       C.cast(lib().fx_plan_batch_begin, C.c_void_p).value, C.cast(lib().fx_plan_batch_end, C.c_void_p).value)
        except ImportError:
            _FXHOST = False
    return _FXHOST


def _pack_predictions_dict(predictions: dict, n_samples: int, max_obstacles: int):
    """The whole predictions dict in one call: walked in C (buffer protocol), packed by fx_pack_predictions.  None when some
    entry is not a contiguous float64 array (the caller converts and takes the general path)."""
    h = _fxhost()
    if not h:
        return None
    try:
        r = h[0].pack_predictions(h[1], predictions, int(n_samples), int(max_obstacles))
    except ValueError as e:
        if b"singular" in lib().fx_last_error():
            raise np.linalg.LinAlgError("Singular matrix") from e
        raise
    if r is None:
        return None
    K, P, out, cnt = r
    o = np.frombuffer(out, dtype=np.float64)
    c = np.frombuffer(cnt, dtype=np.int32)
    n_pos, n_cov = 2 * K * P, 4 * K * P
    return dict(K=K, P=P, pos=o[:n_pos].reshape(K, P, 2), cov_inv=o[n_pos:n_pos + n_cov].reshape(K, P, 4), npred=c[:K],
                hull=o[n_pos + n_cov:].reshape(K, P - 1, 6), nhull=c[K:])


build_obstacle_hulls.pack = _pack_predictions_c
build_obstacle_hulls.pack_dict = _pack_predictions_dict
build_obstacle_hulls.batch = _build_obstacle_hulls_batch
build_obstacle_hulls.invert_cov2 = invert_cov2


def build_boundary_bins(ref_xy, segments, max_len: float, reach: float):
    """fx_build_boundary_bins (host geometry of the library): pieces [n][4], bins [M+1], items."""
    ref = np.ascontiguousarray(ref_xy, dtype=np.float64)
    rx, ry = np.ascontiguousarray(ref[:, 0]), np.ascontiguousarray(ref[:, 1])
    seg = np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 4)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    n_piece, n_item = C.c_int32(0), C.c_int32(0)
    piece = np.zeros((max(len(seg), 1) * 2, 4))
    item = np.zeros(max(len(ref) * 16, 1), dtype=np.int32)
    bins = np.zeros(len(ref) + 1, dtype=np.int32)
    for _ in range(3):
        rc = lib().fx_build_boundary_bins(len(ref), rx.ctypes.data_as(pd), ry.ctypes.data_as(pd), len(seg), seg.ctypes.data_as(pd),
                                          float(max_len), float(reach), len(piece), piece.ctypes.data_as(pd), C.byref(n_piece),
                                          bins.ctypes.data_as(pi), len(item), item.ctypes.data_as(pi), C.byref(n_item))
        if rc == 0:
            return piece[:n_piece.value].copy(), bins, item[:n_item.value].copy()
        if n_piece.value > len(piece):
            piece = np.zeros((n_piece.value, 4))
        elif n_item.value > len(item):
            item = np.zeros(n_item.value, dtype=np.int32)
        else:
            check(rc)
    check(rc)


def effective_cost_names(cost_names, resp: bool = False):
    """The names of an agent's effective cost list: the step's own `cost_names`, with "responsibility" at
    its sorted place -- in front of the first name behind "prediction", else at the end (fx_resp_term_at) -- when a responsibility
    row is given.  None stays None."""
    if cost_names is None:
        return None
    names = list(cost_names)
    if resp:
        if "responsibility" in names:
            raise ValueError("the step's cost list already has a responsibility term")
        at = next((k for k, n in enumerate(names) if _abi.COST_ID[n] > _abi.COST_ID["prediction"]), len(names))
        names.insert(at, "responsibility")
    return names


def rescore_weights(weights, cost_names, resp: bool = False) -> np.ndarray:
    """The [W][n_cost] float64 array FrenetEngine.rescore hands to the library (no device needed).  `weights`: an [W][n_cost] array
    (or one [n_cost] vector) in `cost_names` order, or name -> weight dicts (one, or a sequence) whose non-zero names are exactly
    `cost_names` -- a zero entry is a term upstream does not register (cost_function.py:55-60), so it may be listed, and a step
    whose list lacks a non-zero name, or has one the dict lacks, is another cost function: ValueError.  Every weight is finite and
    not zero (ValueError); negative weights are legal.  cost_names None: no step to compare with, arrays pass as they are.
    resp: the weights are held to `effective_cost_names(cost_names, True)` -- one more entry, "responsibility"."""
    cost_names = effective_cost_names(cost_names, resp)
    if isinstance(weights, dict):
        weights = [weights]
    if not isinstance(weights, np.ndarray) and len(weights) > 0 and all(isinstance(d, dict) for d in weights):
        if cost_names is None:
            raise ValueError("weight dicts need a plan step whose cost_names they are held to")
        rows = []
        for k, d in enumerate(weights):
            mine = sorted(n for n, v in d.items() if v != 0)
            if mine != sorted(cost_names):
                raise ValueError(f"weight set {k}: non-zero terms {mine} are not the step's {sorted(cost_names)}")
            rows.append([d[n] for n in cost_names])
        w = np.array(rows, dtype=np.float64).reshape(len(rows), len(cost_names))
    else:
        try:
            w = np.array(weights, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"weights: an [W][n_cost] array or name -> weight dicts ({e})") from e
        if w.ndim == 1 and w.size > 0:
            w = w[None, :]
    if w.ndim != 2 or w.shape[0] < 1:
        raise ValueError(f"weights of shape {w.shape}: [W][n_cost] with W >= 1")
    if cost_names is not None and w.shape[1] != len(cost_names):
        raise ValueError(f"weights of shape {w.shape}: the step has {len(cost_names)} cost terms {list(cost_names)}")
    if not np.all(np.isfinite(w)) or np.any(w == 0.0):
        raise ValueError("weights must be finite and not zero (a zero weight is another cost list: plan a step with it)")
    return np.ascontiguousarray(w)


def _rescore_row(row, n: int, what: str):
    """a row [n] of FrenetEngine.rescore from outside the step, as the library reads it; None stays None"""
    if row is None:
        return None
    row = np.ascontiguousarray(row, dtype=np.float64)
    if row.shape != (n,):
        raise ValueError(f"{what} of shape {row.shape} for {n} candidates")
    return row


class WinnerPackage:
    """The chosen trajectory as the library packaged it (fx_read_package): `block` [FX_PKG_ROWS][S] = the 14 planes, yaw rate,
    steering angle, shifted heading; coefficients, raw partial costs, cost, flag word, horizon, global index."""

    def __init__(self, pkg: _abi.FxPackage, block: np.ndarray, inputs: PlanInputs):
        self.block = block
        self.index = pkg.index
        self.cost = pkg.cost
        self.flags = pkg.flags
        self.traj_len = pkg.traj_len
        self.tau_lat = pkg.tau_lat   # delta_tau of the lateral polynomial (reactive_planner.py:161-171)
        self._pkg = pkg
        self._costmap = bool(inputs.write_costmap)

    @property
    def lon(self) -> np.ndarray:
        return np.array(self._pkg.coeff_lon)

    @property
    def lat(self) -> np.ndarray:
        return np.array(self._pkg.coeff_lat)

    @property
    def raw_costs(self):
        return np.array(self._pkg.raw_costs[:self._pkg.n_cost]) if self._costmap else None

    def raw_cost_list(self):
        return list(self._pkg.raw_costs[:self._pkg.n_cost]) if self._costmap else None

    @property
    def planes(self) -> np.ndarray:
        return self.block[:_abi.FX_NUM_PLANES]


def math_selftest(x: np.ndarray):
    """(atan, sin, cos) of the device math kernels for the values in x."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    outs = [np.zeros_like(x) for _ in range(3)]
    check(lib().fx_math_selftest(x.size, x.ctypes.data_as(C.POINTER(C.c_double)),
                                 *[o.ctypes.data_as(C.POINTER(C.c_double)) for o in outs]))
    return outs


# fx_device_selftest: op code, doubles per element of each input array, number of outputs (include/fxplan.h)
SELFTEST_OPS = {
    "atan": (0, (1,), 1), "atan_tab": (1, (1,), 1), "atan_small": (2, (1,), 1), "atan_small_tab": (3, (1,), 1),
    "sincos": (4, (1,), 2), "sincos_tab": (5, (1,), 2), "rcp_nr": (6, (1,), 1), "rcp_pred": (7, (1,), 1), "fdiv": (8, (1, 1), 1),
    "sqrt_rsqrt": (9, (1,), 2), "div_rcp": (10, (1, 1), 1), "np_round5": (11, (1,), 1), "wrap_pm_2pi": (12, (1,), 1),
    "obb_hull": (13, (4, 4, 2), 6), "obb_overlap": (14, (6, 6), 1),
}


def device_selftest(op, *arrays):
    """One arithmetic primitive of the kernels (csrc/fx_math.h, fx_walk.h, fx_eval_kernel.h) on the device, elementwise over the
    rows of `arrays`: the list of its output arrays.  `op` is a name of SELFTEST_OPS; an input of width w is [n] (w = 1) or [n][w]."""
    code, widths, n_out = SELFTEST_OPS[op]
    if len(arrays) != len(widths):
        raise ValueError(f"{op} takes {len(widths)} arrays")
    ins = [np.ascontiguousarray(a, dtype=np.float64) for a in arrays]
    n = ins[0].shape[0] if ins[0].ndim else 0
    for a, w in zip(ins, widths):
        if a.shape != ((n,) if w == 1 else (n, w)):
            raise ValueError(f"{op}: input of shape {a.shape}, expected {(n,) if w == 1 else (n, w)}")
    outs = [np.zeros(n) for _ in range(n_out)]
    pd = C.POINTER(C.c_double)
    check(lib().fx_device_selftest(code, n, (pd * 4)(*[a.ctypes.data_as(pd) for a in ins]),
                                   (pd * 6)(*[o.ctypes.data_as(pd) for o in outs])))
    return outs


def device_count() -> int:
    n = C.c_int32(0)
    lib().fx_device_count(C.byref(n))
    return n.value


# -- marshalling of FrenetEngine's pass wrappers: every rule once, for the per-agent and the batched entry of a pass (DESIGN.md
#    section 26); the rules that need the last upload are the private methods at the head of their section of the class --
_PI32, _PI64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _ptr(a, typ=C.c_void_p):
    """an array as the library takes it, NULL for None (`typ`: the pointer type of an entry point declared with one)"""
    return None if a is None else a.ctypes.data_as(typ)


def _bind(out, arrays: dict):
    """the fields of an output structure pointed at the arrays of their names; `out`"""
    for k, a in arrays.items():
        setattr(out, k, a.ctypes.data)
    return out


# candidate rows (candidates, materialise)
def _rows_dict(planes, co, tl, raw, cost, flags, bst) -> dict:
    """the dict of `FrenetEngine.candidates` over the row buffers of `_read_rows`; a part without a buffer is None"""
    lon, lat, tau = (None, None, None) if co is None else (co[:, :6], co[:, 6:12], co[:, 12])
    return dict(planes=planes, lon=lon, lat=lat, tau_lat=tau, traj_len=tl, raw_costs=raw, cost=cost, flags=flags, boundary_step=bst)


# hypotheses
def _pack_hypothesis(dst, s, K: int, P: int, keep: list):
    """One prediction set `s` into the FxHypothesis `dst` of an upload with K obstacles and P predictions: re-strided by
    `hypothesis_arrays` unless it has that K and P and hulls, every array held to its size; the arrays go to `keep`."""
    if K <= 0:   # (an upload without obstacles: the library refuses the call, whatever the sets hold)
        return
    if int(s["K"]) != K or int(s["P"]) != P or not np.size(s.get("hull", ())):
        s = hypothesis_arrays(s, K, P)
    for field, typ, size in (("pos", np.float64, 2 * K * P), ("cov_inv", np.float64, 4 * K * P), ("npred", np.int32, K),
                             ("hull", np.float64, 6 * K * (P - 1)), ("nhull", np.int32, K)):
        a = np.ascontiguousarray(s[field], dtype=typ)
        if a.size != size:
            raise ValueError(f"hypothesis array of {a.size} values, the upload's K={K}, P={P} need {size}")
        keep.append(a)
        setattr(dst, "obs_" + field, a.ctypes.data)


def _hypothesis_outputs(pairs: int, cells_shape, pred: bool, totals: bool, collisions: bool):
    """(arrays by field name, the FxHypothesisOutputs bound to them) of a hypotheses call: winner, cost, n_collisions [pairs], and of
    pred, total (f64) and collision (u8), each of `cells_shape`, the ones asked for -- the others None, and NULL to the library"""
    res = dict(winner=np.empty(pairs, np.int64), cost=np.empty(pairs), n_collisions=np.empty(pairs, np.int64),
               pred=np.empty(cells_shape) if pred else None, total=np.empty(cells_shape) if totals else None,
               collision=np.empty(cells_shape, np.uint8) if collisions else None)
    return res, _bind(_abi.FxHypothesisOutputs(), {k: a for k, a in res.items() if a is not None})


# the risk family (risk, risk_detail, risk_costs, responsibility_cost, prediction_probability)
_RISK_ROWS = ["ego_risk", "obst_risk", "obst_harm_occ"]                                   # [n]
_RISK_COLS = ["ego_risk_max", "obst_risk_max", "ego_harm_max", "obst_harm_max"]           # [K, n] to the library, [n, K] views back
_RISK_COST_ROWS = list(_abi.RISK_COST_NAMES) + ["total", "boundary_harm"]                 # [n], with cost parameters only
_RESP_ROWS = ("resp", "total", "ego_risk", "obst_risk")


def _broadcast_params(x, typ, n: int) -> list:
    """one structure for all listed agents, or one per listed agent: the list"""
    return [x] * n if isinstance(x, typ) else list(x)


def _id_tables(ids, n: int):
    """The id lists of a batched risk call (None: no agent has one; per agent None, every candidate, or an int array) -> (the lists
    as int64 arrays, n_ids [n + 1] with a trailing 0 and the table of pointers as the library takes them, both NULL when no agent
    has a list, what must stay alive behind them).  The caller holds len(lists) to its agent count."""
    ids = [None] * n if ids is None else [None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in ids]
    if all(x is None for x in ids):
        return ids, (None, None), None
    n_ids = np.array([0 if x is None else len(x) for x in ids] + [0], dtype=np.int64)
    backs = [None if x is None else (x if len(x) else np.zeros(1, np.int64)) for x in ids]   # (an empty list is a list: never NULL)
    idp = (_PI64 * len(ids))(*[C.cast(None, _PI64) if x is None else x.ctypes.data_as(_PI64) for x in backs])
    return ids, (_ptr(n_ids, _PI64), idp), (n_ids, backs)


def _check_responsibility_length(cp, K: int, who: str = ""):
    lens = getattr(cp, "_lengths", {})
    if lens.get("responsibility", K) != K:
        raise ValueError(f"{who}responsibility has {lens['responsibility']} entries for {K} obstacles")


def _check_risk_cost_lengths(cp, n: int, K: int, who: str = ""):
    """the arrays behind the pointers of the cost parameters `cp` (None: none) cover what the library reads: [n] and [K]"""
    lens = getattr(cp, "_lengths", {})
    if lens.get("boundary_harm", n) != n:
        raise ValueError(f"{who}boundary_harm has {lens['boundary_harm']} entries for {n} candidates")
    _check_responsibility_length(cp, K, who)


def _check_responsibility(cp, weight, K: int, who: str = ""):
    """The refusals of `responsibility_cost`, in this order and before any library call.  The library refuses the last two as well:
    here they are refused before the probability pass is launched."""
    _check_responsibility_length(cp, K, who)
    if not float(weight) or np.isnan(float(weight)):
        raise ValueError(f"{who}responsibility weight {weight!r}: a non-zero number")
    if cp.responsibility_mode not in (_abi.FX_RISK_RESP_ACTION_SPACE, _abi.FX_RISK_RESP_REACH_SET):
        raise ValueError(f"{who}responsibility_mode {cp.responsibility_mode}: the action-space factors or 'reach_set'")


def _resp_cost_params(cp, weight, pred):
    """FxRespCostParams of one agent: pred None or its [n] prediction entries (no row: NULL, the step's own are summed)"""
    return _abi.FxRespCostParams(float(weight), int(cp.responsibility_mode), cp.responsibility,
                                 pred.ctypes.data if pred is not None and len(pred) else None)


class FrenetEngine(StepRegistry):
    def __init__(self, max_candidates: int, max_steps: int = 30, max_ref_knots: int = 1024, max_obstacles: int = 32,
                 max_pred_steps: int = 64, device: int = 0, max_agents: int = 1):
        self._ctx = C.c_void_p()
        self._inputs: List[PlanInputs] = []
        self._resident_key = None
        self._resident_keys = None
        self.packaging = False
        self.sort_serials = {}   # agent -> sorts of that agent so far (PlanStepResult.ranked_ids: is the agent's device order still mine?)
        self._risk_K = {}        # agent -> K of its `set_risk_obstacles` (shape of the risk passes' [n, K] columns)
        check(lib().fx_create_batch(C.byref(self._ctx), device, max_agents, int(max_candidates), int(max_steps),
                                    int(max_ref_knots), int(max_obstacles), int(max_pred_steps)))
        self.device = device
        self.max_agents = max_agents

    # -- lifetime --
    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            try:
                if self._steps:   # samples somebody still holds read this context's buffers: the last moment to bring them over
                    self.rescue_steps()
            finally:              # (a failed read must not leak the context)
                lib().fx_destroy(self._ctx)
                self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, hip_stream_ptr: int):
        """Run on an external HIP stream (e.g. torch.cuda.current_stream().cuda_stream)."""
        check(lib().fx_set_stream(self._ctx, C.c_void_p(hip_stream_ptr)))

    def set_tuning(self, lanes_per_candidate: int = 0, waves_per_simd: int = 0, kernel_variant: int = 0,
                   block_size: int = 0, mapping: int = 0):
        """Override the automatic work decomposition (0 = automatic; kernel_variant 1 = generic, 2 = grid;
        block_size 64/128/256 lanes for the grid kernel); results are unaffected."""
        check(lib().fx_set_tuning(self._ctx, int(lanes_per_candidate), int(waves_per_simd), int(kernel_variant)))
        check(lib().fx_set_block_size(self._ctx, int(block_size)))
        check(lib().fx_set_part_mapping(self._ctx, int(mapping)))

    def set_store_mode(self, mode: int = 0):
        """Plane stores of the bundle: 0 auto, 1 write-back, 2 write-through (agent scope); results are unaffected."""
        check(lib().fx_set_store_mode(self._ctx, int(mode)))

    def set_winner_buffer(self, d_ptr: int):
        """Device buffer [n_agents][2] (cost f64, global index i64) every step's winner is also written to."""
        check(lib().fx_set_winner_buffer(self._ctx, C.c_void_p(d_ptr)))

    def publish(self, d_ptr: int, n: int):
        """Enqueue the copy of n doubles at device address d_ptr into the pinned publication block."""
        check(lib().fx_publish(self._ctx, C.c_void_p(d_ptr), int(n)))
        self._pub_n = int(n)

    def wait_published(self) -> np.ndarray:
        out = np.empty(self._pub_n)
        check(lib().fx_wait_published(self._ctx, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def set_fused_selection(self, enabled):
        """Selection fused into the evaluation kernel (fx_set_fused_selection; default on): the agent's last workgroup reduces
        the arg-min partials, counts the collisions in front of the winner (agents of at most 8 192 candidates whose obstacle
        stage runs in the evaluation kernel), gathers the winner package and publishes -- one launch per step.  False / 0: always
        the separate selection kernel; 2: in-kernel whatever the candidate count.  Takes effect at the next upload."""
        check(lib().fx_set_fused_selection(self._ctx, 2 if enabled == 2 else int(bool(enabled))))

    def set_obstacle_stage(self, stage: int = 0, steps_per_item: int = 0):
        """Where the obstacle stage runs: 0 auto, 1 fused into the walk, 2 its own (candidate x step)-parallel kernel
        (fx_set_obstacle_stage; steps_per_item 0 auto / 2 / 3 / 5); takes effect at the next upload.  Decisions are unaffected."""
        check(lib().fx_set_obstacle_stage(self._ctx, int(stage), int(steps_per_item)))
        self._resident_key = None   # the decomposition is chosen at upload time
        self._resident_keys = None

    def set_step_kernel(self, mode: int = 0, steps_per_item: int = 0):
        """The whole plan step in ONE launch (fx_set_step_kernel, csrc/fx_step_kernel.h), opt-in: 0 / 1 off (walk, obstacle kernel,
        selection as three launches -- faster on the MI355X), 2 on where applicable; steps_per_item 0 auto / 3 / 5 / 8.  Takes effect
        at the next upload.  Same results (bit for bit at three steps per item)."""
        check(lib().fx_set_step_kernel(self._ctx, int(mode), int(steps_per_item)))
        self._resident_key = None
        self._resident_keys = None

    def step_info(self) -> dict:
        """how the last evaluation was launched (fx_step_info_ex)"""
        v = np.zeros(16, np.int64)
        check(lib().fx_step_info_ex(self._ctx, v.ctypes.data))
        keys = ("grid_kernel", "lanes_per_candidate", "waves_per_simd", "block", "wave_split", "fused_selection", "blocks", "agents",
                "package", "lds_bytes", "obstacle_kernel", "obstacle_steps_per_item", "obstacle_items", "obstacle_lds_bytes",
                "obstacle_workgroup_waves", "tail")
        info = dict(zip(keys, (int(x) for x in v)))
        # [15]: bits 0-1 what the agent's last workgroup did (fx_tail.h), bits 8-9 how the latest inputs reached the device:
        # 1 DMA copy, 2 staging kernel, 3 written by the host into device memory (large BAR)
        info["staging"] = ("none", "dma", "kernel", "host_writes")[(info["tail"] >> 8) & 3]
        info["step_kernel"] = (info["tail"] >> 16) & 1   # the whole step ran as ONE launch (fx_step_kernel.h)
        info["tail"] &= 0xff
        return info

    def obstacle_kernel_times(self, max_n: int = 256):
        """obstacle-kernel ms of the most recent timed steps, oldest first (0 where the stage ran fused)"""
        ob = np.zeros(max_n, dtype=np.float64)
        n = C.c_int32(0)
        check(lib().fx_read_obstacle_kernel_times(self._ctx, max_n, ob.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return ob[:n.value]

    @property
    def last_obstacle_kernel_ms(self) -> float:
        return float(lib().fx_last_obstacle_kernel_ms(self._ctx))

    TIMING = {"off": 0, "stream": 1, "kernel": 2}

    def set_timing(self, mode, every: int = 1):
        """HIP-event timing of (every n-th) step: "off" / False (default), "stream" / True (stream events around the
        kernels) or "kernel" (events attached to the evaluation kernel itself -- what a kernel trace reports).
        Times are read lazily: `last_kernel_ms`, `last_eval_kernel_ms`, `kernel_times()`."""
        if isinstance(mode, str):
            mode = self.TIMING[mode]
        check(lib().fx_set_timing(self._ctx, int(mode)))
        check(lib().fx_set_timing_interval(self._ctx, int(every)))

    def kernel_times(self, max_n: int = 256):
        """(evaluation-kernel ms, whole-step device ms) of the most recent timed steps, oldest first."""
        ev = np.zeros(max_n, dtype=np.float64)
        st = np.zeros(max_n, dtype=np.float64)
        n = C.c_int32(0)
        check(lib().fx_read_kernel_times(self._ctx, max_n, ev.ctypes.data_as(C.POINTER(C.c_double)),
                                         st.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return ev[:n.value], st[:n.value]

    # -- plan step, split so callers can overlap host work (upload/evaluate enqueue only) --
    def upload(self, inputs):
        if self._steps:
            self.rescue_steps()
        batch = list(inputs) if isinstance(inputs, (list, tuple)) else [inputs]
        self._inputs = batch
        self._resident_key = None
        self._resident_keys = None
        arr = (_abi.FxProblem * len(batch))(*[b.as_struct() for b in batch])
        self._structs = arr  # keep pointers alive until the copy has been enqueued (h2d staging is synchronous memcpy)
        check(lib().fx_upload_batch(self._ctx, len(batch), arr))

    @staticmethod
    def make_state_update(x0_lon=None, x0_lat=None, x0_orientation=None, v_des=None, low_vel_mode=None, t_samp=None,
                          v_samp=None, d_samp=None, obstacles=None):
        """FxStateUpdate (+ the arrays it points into) for `update_state`: what changes between two plan steps of a
        planner that keeps its reference path, grid shape and cost function.  `obstacles` = a packed predictions dict
        (problem.pack_predictions) with the K and P of the upload.  Build it once, reuse it as often as wanted."""
        u = _abi.FxStateUpdate()
        keep = []

        def arr(a, typ=np.float64):
            a = np.ascontiguousarray(a, dtype=typ)
            keep.append(a)
            return a.ctypes.data

        if x0_lon is not None: u.x0_lon = arr(x0_lon)
        if x0_lat is not None: u.x0_lat = arr(x0_lat)
        u.x0_orientation = float("nan") if x0_orientation is None else float(x0_orientation)
        u.v_des = float("nan") if v_des is None else float(v_des)
        u.low_vel_mode = -1 if low_vel_mode is None else int(bool(low_vel_mode))
        # (the shapes travel with the pointers: fx_update_state refuses arrays that are not the upload's size)
        if t_samp is not None: u.t_samp, u.nT = arr(t_samp), len(keep[-1])
        if v_samp is not None: u.v_samp, u.nV = arr(v_samp), len(keep[-1])
        if d_samp is not None: u.d_samp, u.nD = arr(d_samp), len(keep[-1])
        if obstacles is not None and obstacles["K"] > 0:
            u.K, u.P = int(obstacles["K"]), int(obstacles["P"])
            if np.shape(obstacles["pos"]) != (u.K, u.P, 2) or np.size(obstacles["cov_inv"]) != 4 * u.K * u.P \
                    or np.size(obstacles["npred"]) != u.K:
                raise ValueError("packed predictions: array shapes do not match their K / P")
            u.obs_pos, u.obs_cov_inv = arr(obstacles["pos"]), arr(obstacles["cov_inv"])
            u.obs_npred = arr(obstacles["npred"], np.int32)
            if obstacles.get("hull") is not None and obstacles["hull"].size:  # also when no hull is left: the old ones must go
                u.obs_hull, u.obs_nhull = arr(obstacles["hull"]), arr(obstacles["nhull"], np.int32)
        u._keep = keep
        return u

    @staticmethod
    def _state_update_of(inp: PlanInputs, u=None):
        """FxStateUpdate straight from a PlanInputs (its arrays are contiguous float64 / int32 already: no conversions); the
        addresses are taken in C (`_fxhost.state_update`: ten `array.ctypes.data` look-ups cost 8 us of a plan step)"""
        if u is None:
            u = _abi.FxStateUpdate()
        o = inp.obstacles
        h = _fxhost()
        if h:
            try:
                k = o["K"] > 0
                hull = k and o["hull"].size > 0
                h[0].state_update(C.addressof(u), inp.x0_lon, inp.x0_lat, float(inp.x0_orientation), float(inp.v_des),
                                  int(bool(inp.low_vel_mode)), inp.t_samp, inp.v_samp, inp.d_samp,
                                  o["pos"] if k else None, o["cov_inv"] if k else None, o["npred"] if k else None,
                                  o["hull"] if hull else None, o["nhull"] if hull else None)
                u._keep = inp   # the arrays live as long as the inputs do
                return u
            except (TypeError, ValueError, BufferError):
                C.memset(C.addressof(u), 0, C.sizeof(u))   # something is not a plain contiguous array: the long way
        u.x0_lon, u.x0_lat = inp.x0_lon.ctypes.data, inp.x0_lat.ctypes.data
        u.x0_orientation, u.v_des, u.low_vel_mode = float(inp.x0_orientation), float(inp.v_des), int(bool(inp.low_vel_mode))
        u.t_samp, u.v_samp, u.d_samp = inp.t_samp.ctypes.data, inp.v_samp.ctypes.data, inp.d_samp.ctypes.data
        u.nT, u.nV, u.nD = len(inp.t_samp), len(inp.v_samp), len(inp.d_samp)
        if o["K"] > 0:
            u.K, u.P = int(o["K"]), int(o["P"])
            if o["pos"].shape != (u.K, u.P, 2) or o["cov_inv"].size != 4 * u.K * u.P or o["npred"].size != u.K:
                raise ValueError("packed predictions: array shapes do not match their K / P")
            u.obs_pos, u.obs_cov_inv, u.obs_npred = o["pos"].ctypes.data, o["cov_inv"].ctypes.data, o["npred"].ctypes.data
            if o["hull"].size:
                u.obs_hull, u.obs_nhull = o["hull"].ctypes.data, o["nhull"].ctypes.data
        u._keep = inp   # the arrays live as long as the inputs do
        return u

    def update_state(self, update, agent: int = 0):
        """Rewrite the step-dependent inputs of one uploaded agent in place (fx_update_state): one small host-to-device
        copy in front of the next evaluation instead of a full upload."""
        check(lib().fx_update_state(self._ctx, int(agent), C.byref(update)))

    def update_step_raw(self, update):
        """update_state(agent 0) + step_raw() in ONE call across the boundary"""
        if self._steps:
            self.rescue_steps()
        res = getattr(self, "_res_buf", None)
        if res is None or len(res) != len(self._inputs):
            res = self._res_buf = (_abi.FxResult * len(self._inputs))()
        check(lib().fx_update_step(self._ctx, C.byref(update), res))
        return res

    def evaluate(self):
        if self._steps:
            self.rescue_steps()
        check(lib().fx_evaluate(self._ctx))

    def finish(self):
        n = len(self._inputs)
        res = (_abi.FxResult * n)()
        check(lib().fx_finish_batch(self._ctx, res))
        out = [r.as_dict() for r in res]
        return out

    def step_raw(self):
        """evaluate() + finish() for the resident inputs in ONE call across the boundary; returns the FxResult array
        (fields as attributes: best_index, best_cost, n_feasible, ...) without building Python dicts."""
        if self._steps:
            self.rescue_steps()
        n = len(self._inputs)
        res = getattr(self, "_res_buf", None)
        if res is None or len(res) != n:
            res = self._res_buf = (_abi.FxResult * n)()
        check(lib().fx_step(self._ctx, res))
        return res

    def plan_step(self, inputs: PlanInputs) -> dict:
        if self._steps:
            self.rescue_steps()
        self.upload(inputs)
        self.evaluate()
        return self.finish()[0]

    def plan_step_packaged(self, inputs: PlanInputs, yaw_rate0: float = 0.0):
        """A planner's closed-loop plan step in ONE call across the boundary (fx_plan_and_package): when the resident upload
        has the structure of `inputs` (PlanInputs.structure_key) only the ego state, sampling values and predictions are
        rewritten in place, else everything is uploaded; evaluation; result; the winner's arrays, which the device gathers
        into pinned host memory behind the selection.  Returns (result dict, WinnerPackage or None)."""
        if self._steps:
            self.rescue_steps()
        key = inputs.structure_key()
        upd = None
        h = _fxhost()
        if h and inputs.sampling_matrix is None and self._resident_key == key and len(self._inputs) == 1 and inputs.write_bundle:
            # the closed loop's usual step through the extension (fx_plan_batch_packaged with one agent): the inputs' arrays are
            # read in C, the result comes back as a dict -- no struct filling, no per-field conversion on this side
            self._inputs = [inputs]
            pkgs = (_abi.FxPackage * 1)()
            block = np.empty((1, _abi.FX_PKG_ROWS, inputs.n_samples))
            out = h[0].plan_batch(h[2], self._ctx.value, self._inputs, (float(yaw_rate0),), block, C.addressof(pkgs), True)
            if out.__class__ is int:
                check(out)
            return out[0], (WinnerPackage(pkgs[0], block[0], inputs) if pkgs[0].found else None)
        if inputs.sampling_matrix is None and self._resident_key == key and len(self._inputs) == 1:
            upd = getattr(self, "_upd", None)
            if upd is None:
                upd = self._upd = _abi.FxStateUpdate()   # consumed inside the call below: one struct per engine
            upd = self._state_update_of(inputs, upd)
            self._inputs = [inputs]
        else:
            self.upload(inputs)
            self._resident_key = key
        res = (_abi.FxResult * 1)()
        pkg = _abi.FxPackage()
        block = np.empty((_abi.FX_PKG_ROWS, inputs.n_samples))
        check(lib().fx_plan_and_package(self._ctx, C.byref(upd) if upd is not None else None, float(yaw_rate0), res,
                                        C.byref(pkg), block.ctypes.data))
        return res[0].as_dict(), (WinnerPackage(pkg, block, inputs) if pkg.found else None)

    # -- survivor exchange inside the library (fx_comm_*) --
    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the 128-byte id every rank hands to comm_init (broadcast it with whatever the program has)"""
        buf = (C.c_uint8 * 128)()
        check(lib().fx_comm_unique_id(C.addressof(buf)))
        return bytes(buf)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(lib().fx_comm_init(self._ctx, C.addressof(buf), int(rank), int(world)))
        self._comm_world = int(world)
        self._comm_agents = int(self.max_agents)   # (fx_comm_init's default; comm_set_agents changes it)

    def comm_check(self, world: int) -> bool:
        """Local preconditions of comm_init (RCCL present, capacity), nothing collective: the ranks agree on the answer
        BEFORE any of them calls comm_init (fx_comm_check)."""
        return lib().fx_comm_check(self._ctx, int(world)) == 0

    def set_timeout_ms(self, timeout_ms: int):
        """Bound of every host wait on device work (default 20 000 ms, the reference's TIMEOUT); FxTimeoutError beyond it."""
        check(lib().fx_set_timeout_ms(self._ctx, int(timeout_ms)))

    def comm_set_agents(self, n_agents: int):
        """The agent rows every rank contributes to an exchange (fx_comm_set_agents): the ranks agree on it beforehand."""
        check(lib().fx_comm_set_agents(self._ctx, int(n_agents)))
        self._comm_agents = int(n_agents)

    def set_exchange_mode(self, mode: int):
        """0: the library's all-gather lands in device memory and a publication kernel copies it out; 1: it lands straight in the
        pinned block and a stream-ordered write signals it (fx_set_exchange_mode)."""
        check(lib().fx_set_exchange_mode(self._ctx, int(mode)))
        self._exchange_mode = int(mode)

    def comm_info(self) -> dict:
        """rank, world, the rank count RCCL itself reports (ncclCommCount; -1 if unavailable), agent rows per rank"""
        v = (C.c_int32 * 4)()
        check(lib().fx_comm_info(self._ctx, v))
        return dict(rank=int(v[0]), world=int(v[1]), rccl_ranks=int(v[2]), agent_rows=int(v[3]))

    def step_exchange_topk_raw(self, k: int):
        """evaluate + per-agent top-k + ONE all-gather + finish in one call (fx_step_exchange_topk):
        (FxResult array, cost [W, A, k], index [W, A, k]) with A = the communicator's agent rows (comm_set_agents)"""
        if self._steps:
            self.rescue_steps()
        n, A = len(self._inputs), self._comm_agents
        res = getattr(self, "_res_buf", None)
        if res is None or len(res) != n:
            res = self._res_buf = (_abi.FxResult * n)()
        x = getattr(self, "_xchg_topk", None)
        if x is None or x[0].shape != (self._comm_world, A, k):
            x = self._xchg_topk = (np.empty((self._comm_world, A, k)), np.empty((self._comm_world, A, k), np.int64))
        check(lib().fx_step_exchange_topk(self._ctx, int(k), res, x[0].ctypes.data, x[1].ctypes.data))
        return res, x[0], x[1]

    def comm_destroy(self):
        check(lib().fx_comm_destroy(self._ctx))
        self._comm_world = 0

    def step_exchange_raw(self):
        """evaluate + all-gather of every rank's winner(s) + finish in ONE call: (FxResult array, cost [W, A], index [W, A]) with
        A = the communicator's agent rows (comm_set_agents; rows a rank does not fill say cost inf / index -1)"""
        if self._steps:
            self.rescue_steps()
        n, A = len(self._inputs), self._comm_agents
        res = getattr(self, "_res_buf", None)
        if res is None or len(res) != n:
            res = self._res_buf = (_abi.FxResult * n)()
        x = getattr(self, "_xchg_buf", None)
        if x is None or x[0].shape != (self._comm_world, A):
            x = self._xchg_buf = (np.empty((self._comm_world, A)), np.empty((self._comm_world, A), np.int64))
        check(lib().fx_step_exchange(self._ctx, res, x[0].ctypes.data, x[1].ctypes.data))
        return res, x[0], x[1]

    def set_package(self, enabled: bool):
        """Gather the winner's arrays into pinned host memory behind every evaluation that writes the bundle (fx_set_package);
        read them with `package(agent)` after finish()."""
        check(lib().fx_set_package(self._ctx, int(bool(enabled))))
        self.packaging = bool(enabled)

    def package(self, agent: int = 0, yaw_rate0: float = 0.0):
        pkg = _abi.FxPackage()
        inp = self._inputs[agent]
        block = np.empty((_abi.FX_PKG_ROWS, inp.n_samples))
        check(lib().fx_read_package(self._ctx, int(agent), float(yaw_rate0), C.byref(pkg), block.ctypes.data_as(C.POINTER(C.c_double))))
        return WinnerPackage(pkg, block, inp) if pkg.found else None

    def plan_batch(self, inputs: Sequence[PlanInputs]) -> List[dict]:
        """One batched launch over the agents.  When the resident upload has the same agents' structures
        (PlanInputs.structure_key) only their states, sampling values and predictions are rewritten in place
        (fx_update_state per agent, one staging copy in front of the evaluation); otherwise everything is uploaded."""
        if self._steps:
            self.rescue_steps()
        inputs = list(inputs)
        keys = [inp.structure_key() if inp.sampling_matrix is None else None for inp in inputs]
        if self._resident_keys is not None and keys == self._resident_keys and None not in keys:
            for a, inp in enumerate(inputs):
                self.update_state(self._state_update_of(inp), a)
            self._inputs = inputs
        else:
            self.upload(inputs)
            self._resident_keys = keys
        self.evaluate()
        return self.finish()

    def plan_batch_packaged(self, inputs: Sequence[PlanInputs], yaw_rates: Sequence[float]):
        """plan_batch + every agent's winner package in ONE call across the boundary (fx_plan_batch_packaged through
        `_fxhost.plan_batch`: the inputs' arrays are read in C, the results come back as dicts): ([result dict],
        [WinnerPackage or None]).  The general path -- different structures, a sampling matrix, horizons of different
        lengths, no extension -- is plan_batch() followed by package() per agent."""
        if self._steps:
            self.rescue_steps()
        inputs = list(inputs)
        n = len(inputs)
        keys = [inp.structure_key() if inp.sampling_matrix is None else None for inp in inputs]
        h = _fxhost()
        S = inputs[0].n_samples if n else 0
        fast = bool(h) and n > 0 and None not in keys and all(inp.n_samples == S and inp.write_bundle for inp in inputs)
        if not fast:
            res = self.plan_batch(inputs)
            return res, [self.package(a, yaw_rates[a]) if inputs[a].write_bundle and getattr(self, "packaging", False) else None
                         for a in range(n)]
        update = self._resident_keys is not None and keys == self._resident_keys
        if not update:
            self.upload(inputs)
            self._resident_keys = keys
        else:
            self._inputs = inputs
        pkgs = (_abi.FxPackage * n)()
        blocks = np.empty((n, _abi.FX_PKG_ROWS, S))
        out = h[0].plan_batch(h[2], self._ctx.value, inputs, yaw_rates, blocks, C.addressof(pkgs), update)
        if out.__class__ is int:
            check(out)
        return out, [WinnerPackage(pkgs[a], blocks[a], inputs[a]) if pkgs[a].found else None for a in range(n)]

    def plan_batch_begin(self, inputs: Sequence[PlanInputs]):
        """First half of plan_batch_packaged: the agents' states rewritten in place (or everything uploaded) and the evaluation
        launched -- returns without waiting (fx_plan_batch_begin).  The token goes to plan_batch_end.  None when the batch
        cannot take the packaged path (see plan_batch_packaged): the caller then uses that one."""
        if self._steps:
            self.rescue_steps()
        inputs = list(inputs)
        n = len(inputs)
        h = _fxhost()
        if not h or n == 0 or any(inp.sampling_matrix is not None or not inp.write_bundle for inp in inputs):
            return None
        S = inputs[0].n_samples
        if any(inp.n_samples != S for inp in inputs):
            return None
        keys = [inp.structure_key() for inp in inputs]
        update = self._resident_keys is not None and keys == self._resident_keys
        if not update:
            self.upload(inputs)
            self._resident_keys = keys
        else:
            self._inputs = inputs
        rc = h[0].plan_batch_begin(h[3], self._ctx.value, inputs, update)
        if rc is not None:
            check(rc)
        return (inputs, S)

    def plan_batch_end(self, token, yaw_rates: Sequence[float]):
        """Second half: wait for the evaluation plan_batch_begin launched, ([result dict], [WinnerPackage or None])"""
        inputs, S = token
        n = len(inputs)
        h = _fxhost()
        pkgs = (_abi.FxPackage * n)()
        blocks = np.empty((n, _abi.FX_PKG_ROWS, S))
        out = h[0].plan_batch_end(h[4], self._ctx.value, n, yaw_rates, blocks, C.addressof(pkgs))
        if out.__class__ is int:
            check(out)
        return out, [WinnerPackage(pkgs[a], blocks[a], inputs[a]) if pkgs[a].found else None for a in range(n)]

    # -- read-back --
    def costs(self, agent: int = 0):
        n = self._inputs[agent].n_candidates
        cost = np.zeros(n)
        flags = np.zeros(n, np.uint32)
        check(lib().fx_read_costs_agent(self._ctx, agent, cost.ctypes.data_as(C.POINTER(C.c_double)),
                                        flags.ctypes.data_as(C.POINTER(C.c_uint32))))
        return cost, flags

    def boundary_steps(self, agent: int = 0) -> np.ndarray:
        """first step at which each candidate's footprint meets the road boundary, -1 if never"""
        out = np.zeros(self._inputs[agent].n_candidates, dtype=np.int32)
        check(lib().fx_read_boundary_steps_agent(self._ctx, agent, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def costmap(self, agent: int = 0) -> np.ndarray:
        """[C, n_cost] raw (unweighted) partial costs, columns in inputs.cost_names order."""
        inp = self._inputs[agent]
        raw = np.zeros((max(len(inp.cost_names), 1), inp.n_candidates))
        check(lib().fx_read_costmap_agent(self._ctx, agent, raw.ctypes.data_as(C.POINTER(C.c_double))))
        return np.ascontiguousarray(raw[:len(inp.cost_names)].T)

    def coeffs(self, index: int, agent: int = 0):
        lon, lat = np.zeros(6), np.zeros(6)
        tl = C.c_int32(0)
        check(lib().fx_read_coeffs_agent(self._ctx, agent, int(index), lon.ctypes.data_as(C.POINTER(C.c_double)),
                                         lat.ctypes.data_as(C.POINTER(C.c_double)), C.byref(tl)))
        tau = C.c_double(0.0)
        check(lib().fx_read_lat_tau_agent(self._ctx, agent, int(index), C.byref(tau)))
        return lon, lat, tl.value, tau.value

    def sample(self, index: int, agent: int = 0) -> np.ndarray:
        """[14, S] planes of one candidate (gathered from the SoA bundle)."""
        inp = self._inputs[agent]
        out = np.zeros((_abi.FX_NUM_PLANES, inp.n_samples))
        check(lib().fx_read_sample_agent(self._ctx, agent, int(index), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def candidate(self, index: int, agent: int = 0) -> dict:
        """Everything one trajectory object exposes, with one synchronisation: planes [14, S], lon / lat coefficients,
        the lateral polynomial's delta_tau, traj_len, raw partial costs (inputs.cost_names order), total cost, flag word."""
        inp = self._inputs[agent]
        planes = np.zeros((_abi.FX_NUM_PLANES, inp.n_samples))
        co = np.zeros(13)
        raw = np.zeros(max(len(inp.cost_names), 1))
        tl, cost, flags = C.c_int32(0), C.c_double(0.0), C.c_uint32(0)
        pd = C.POINTER(C.c_double)
        have_b, have_c = bool(inp.write_bundle), bool(inp.write_costmap) and len(inp.cost_names) > 0
        check(lib().fx_read_candidate_agent(self._ctx, agent, int(index), planes.ctypes.data_as(pd) if have_b else None,
                                            co.ctypes.data_as(pd) if have_b else None, C.byref(tl) if have_b else None,
                                            raw.ctypes.data_as(pd) if have_c else None, C.byref(cost), C.byref(flags)))
        return dict(planes=planes if have_b else None, lon=co[:6].copy(), lat=co[6:12].copy(), tau_lat=float(co[12]), traj_len=tl.value,
                    raw_costs=raw[:len(inp.cost_names)] if have_c else None, cost=cost.value, flags=flags.value)

    # -- the agents a pass beside the step means (the wrappers below) --
    def _agent_input(self, agent: int):
        """the agent's inputs of the last upload; None for an agent that is not there (the library refuses the call)"""
        return self._inputs[agent] if 0 <= agent < len(self._inputs) else None

    def _listed(self, agents, n: Optional[int] = None):
        """(the listed agents, their int32 array or None for NULL) of a batched call.  agents None: to the risk family every agent of
        the last upload, in order, and NULL is passed; to a pass with one argument per listed agent (n of them) 0 .. n - 1, passed."""
        if agents is None and n is None:
            return list(range(len(self._inputs))), None
        listed = list(range(n)) if agents is None else [int(a) for a in agents]
        return listed, np.array(listed, np.int32)

    def _row_counts(self, listed, ids=None):
        """(rows per listed agent: its id list, else all its candidates; their offsets [n + 1] in the call's concatenated arrays)"""
        # (an agent the library will refuse counts no rows: the refusal comes before anything is written)
        counts = [inp.n_candidates if inp is not None else 0 for inp in map(self._agent_input, listed)]
        if ids is not None:
            counts = [m if x is None else len(x) for m, x in zip(counts, ids)]
        return counts, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    def _info3(self, fn) -> list:
        """the three int32 a fx_last_*_info entry point writes"""
        v = [C.c_int32(0) for _ in range(3)]
        check(fn(self._ctx, *[C.byref(x) for x in v]))
        return [int(x.value) for x in v]

    def candidates(self, ids, agent: int = 0) -> dict:
        """candidate() for a list of indices in ONE call (fx_read_candidates_agent: a gather kernel behind the step, one copy and
        one synchronisation per chunk of _abi.FX_READ_CHUNK_BYTES): planes [n, 14, S], lon / lat [n, 6], tau_lat [n], traj_len [n],
        raw_costs [n, n_cost], cost [n], flags [n], boundary_step [n], rows in the order of `ids` (any order, duplicates allowed);
        None for the parts the step did not produce."""
        inp = self._inputs[agent]
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        # ascending indices: neighbouring workgroups of the gather then touch neighbouring lines; the rows are permuted back here
        order = None
        if len(ids) > 1 and not bool((ids[1:] >= ids[:-1]).all()):
            order = np.argsort(ids, kind="stable")
            ids = ids[order]
        rows = self._read_rows(lib().fx_read_candidates_agent, ids, agent, bool(inp.write_bundle),
                               bool(inp.write_costmap) and len(inp.cost_names) > 0)
        if order is not None:
            back = np.argsort(order)   # (row order[i] of the result is row i of what was read)
            rows = [None if a is None else a[back] for a in rows]
        return _rows_dict(*rows)

    def _read_rows(self, fn, ids, agent: int, have_b: bool, have_c: bool) -> list:
        """The rows of `ids` read by `fn` (fx_read_candidates_agent, fx_read_materialised_agent): planes, coefficients [n, 13], traj_len
        (None, and NULL to the library, without have_b), raw costs (without have_c), cost, flags, boundary steps (unless the step
        ran the road-boundary stage)."""
        inp = self._inputs[agent]
        n, n_cost = len(ids), len(inp.cost_names)
        have_r = inp._bound is not None and inp._bound["n"] > 0
        rows = [np.empty((n, _abi.FX_NUM_PLANES, inp.n_samples)) if have_b else None, np.empty((n, 13)) if have_b else None,
                np.empty(n, np.int32) if have_b else None, np.empty((n, n_cost)) if have_c else None, np.empty(n), np.empty(n, np.uint32),
                np.empty(n, np.int32) if have_r else None]
        p = [_ptr(a) for a in rows]
        p[3] = p[3] if n_cost > 0 else None   # (no cost term: no raw rows, whatever the buffer)
        check(fn(self._ctx, int(agent), n, _ptr(ids), *p))
        return rows

    def materialise(self, ids, agent: int = 0) -> dict:
        """The dict of `candidates(ids)` with EVERY part filled, whatever the step stored: the listed
        candidates of the last step are re-walked with the step's own arithmetic into the agent's sparse set
        (fx_materialise_candidates_agent) and read back (fx_read_materialised_agent).  Rows in the order of `ids` (any order,
        duplicates allowed); boundary_step None unless the step ran the road-boundary stage.  The set stays on the device until
        the next materialise of this agent or the next evaluation, upload or state update: `risk`, `risk_detail` and
        `risk_costs` of a step without a bundle accept ids inside it, `materialised_package` packages one of its rows.  Nothing
        the step wrote is touched (costs(), topk(), kept samples stay as they were), so no kept step is rescued here."""
        self._inputs[agent]   # (an agent that is not there: IndexError, before the library is asked)
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        check(lib().fx_materialise_candidates_agent(self._ctx, int(agent), len(ids), _ptr(ids)))
        return self._read_materialised(ids, agent)

    def _read_materialised(self, ids, agent: int) -> dict:
        """the rows of `ids` from the agent's sparse set (fx_read_materialised_agent), every part"""
        return _rows_dict(*self._read_rows(lib().fx_read_materialised_agent, ids, agent, True, True))

    def materialised_package(self, index: int, yaw_rate: float = 0.0, agent: int = 0):
        """The winner package of `package()` for candidate `index` of the agent's sparse set (fx_read_package_materialised)"""
        pkg = _abi.FxPackage()
        inp = self._inputs[agent]
        block = np.empty((_abi.FX_PKG_ROWS, inp.n_samples))
        check(lib().fx_read_package_materialised(self._ctx, int(agent), int(index), float(yaw_rate), C.byref(pkg), block.ctypes.data))
        w = WinnerPackage(pkg, block, inp)
        w._costmap = True   # (a set's rows carry their raw costs whatever the step stored)
        return w

    def set_materialise_lanes(self, lanes: int):
        """Lanes per listed candidate of the list kernel (fx_set_materialise_lanes): 0 or 1 one lane (the
        default), 8 or 32 the horizon split over that many adjacent lanes; anything else is refused and the setting stays.
        Applies to `materialise` and `materialise_batch`; an agent with a windowed cost term runs at one lane whatever is set."""
        check(lib().fx_set_materialise_lanes(self._ctx, int(lanes)))

    def materialise_batch(self, ids, agents=None) -> list:
        """`materialise` for several agents of the last step in one call (fx_materialise_candidates_batch): ids[j] is the list of
        agents[j] (None: agent j); an empty list clears that agent's set.  One wait, one upload and one launch per kernel variant
        present, whatever the agent count; every agent gets the set its own `materialise` would have made.  Returns one
        `materialise` dict per listed agent, read back per agent."""
        agents, ag = self._listed(agents, len(ids))
        if len(agents) != len(ids):
            raise ValueError(f"{len(ids)} lists for {len(agents)} agents")
        lists = [np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in ids]
        n = len(agents)
        n_ids = np.asarray([len(x) for x in lists], np.int64)
        addr = np.asarray([x.ctypes.data if len(x) else 0 for x in lists], np.uint64)
        check(lib().fx_materialise_candidates_batch(self._ctx, n, *[_ptr(a) if n else None for a in (ag, n_ids, addr)]))
        return [self._read_materialised(x, a) for x, a in zip(lists, agents)]

    @property
    def last_materialise_ms(self) -> float:
        """device time of the last `materialise` or `materialise_batch` call's list kernels"""
        return float(lib().fx_last_materialise_ms(self._ctx))

    @property
    def last_materialise_info(self) -> dict:
        """the last materialise call (fx_last_materialise_info): lanes (the widest split among its rows), launches, rows"""
        return dict(zip(("lanes", "launches", "rows"), self._info3(lib().fx_last_materialise_info)))

    # -- stable cost order of all candidates, on the device --
    def sort_candidates(self, agent: int = 0, require: int = _abi.FX_FLAG_COSTED, exclude: int = 0):
        """Sort the agent's candidates of the last step by cost on the device (fx_sort_candidates_agent): a stable order, ties and
        NaNs by index, NaNs last -- np.argsort(kind="stable") over the pool (flags & require) == require and (flags & exclude) == 0.
        Returns (n_pool, n_nan): the pool's size and how many of its members have a NaN cost (the last n_nan ranks).  The order
        stays on the device until the next sort of this agent or the next evaluation, upload or state update; `ranked` reads it."""
        n_pool, n_nan = C.c_int64(0), C.c_int64(0)
        check(lib().fx_sort_candidates_agent(self._ctx, int(agent), int(require), int(exclude), C.byref(n_pool), C.byref(n_nan)))
        self.sort_serials[int(agent)] = self.sort_serials.get(int(agent), 0) + 1
        return int(n_pool.value), int(n_nan.value)

    def sort_candidates_batch(self, require: int = _abi.FX_FLAG_COSTED, exclude: int = 0):
        """sort_candidates for every agent of the last step in one launch sequence; returns (n_pool [n_agents], n_nan [n_agents])"""
        n = len(self._inputs)
        n_pool, n_nan = np.zeros(n, np.int64), np.zeros(n, np.int64)
        pi64 = C.POINTER(C.c_int64)
        check(lib().fx_sort_candidates_batch(self._ctx, int(require), int(exclude), n_pool.ctypes.data_as(pi64), n_nan.ctypes.data_as(pi64)))
        for a in range(n):
            self.sort_serials[a] = self.sort_serials.get(a, 0) + 1
        return n_pool, n_nan

    def ranked(self, first: int, n: int, agent: int = 0, with_cost: bool = False):
        """Ranks [first, first + n) of the agent's last sort: indices within the shard (what candidates(), materialise() and the
        risk passes take).  with_cost: (ids, cost, flags), the costs and flag words as the step wrote them, bit for bit."""
        n = int(n)
        inp = self._agent_input(agent)
        room = min(max(n, 0), inp.n_candidates) if inp is not None else 0   # (a longer range is refused)
        ids = np.empty(room, np.int64)
        cost = np.empty(room) if with_cost else None
        flags = np.empty(room, np.uint32) if with_cost else None
        check(lib().fx_read_ranked_agent(self._ctx, int(agent), int(first), n, _ptr(ids), _ptr(cost), _ptr(flags)))
        return (ids, cost, flags) if with_cost else ids

    def sort_view(self, agent: int = 0):
        """(device pointer of the agent's order: int64 local indices by rank, n_pool) of a valid order (fx_sort_views)"""
        p, n_pool = C.c_void_p(), C.c_int64(0)
        check(lib().fx_sort_views(self._ctx, int(agent), C.byref(p), C.byref(n_pool)))
        return p.value, int(n_pool.value)

    @property
    def last_sort_ms(self) -> float:
        """device time of the last sort's launches"""
        return float(lib().fx_last_sort_ms(self._ctx))

    # -- the last step re-scored under other cost weights, on the device (DESIGN.md sections 23 and 24) --
    def _rescore_set(self, weights, agent: int, pred, resp):
        """(weights [W][n_cost] held to the agent's effective cost list, its candidates, pred and resp row held to them)"""
        inp = self._agent_input(agent)
        w = rescore_weights(weights, inp.cost_names if inp is not None else None, resp is not None)
        n = inp.n_candidates if inp is not None else 0
        return w, n, _rescore_row(pred, n, "pred"), _rescore_row(resp, n, "resp")

    def rescore(self, weights, agent: int = 0, totals: bool = False, pred=None, resp=None) -> dict:
        """The agent's last step under W other weight vectors in one call (fx_rescore_agent): which candidate wins, and at what cost,
        had the step run with each of them.  `weights`: [W][n_cost] in the step's `PlanInputs.cost_names` order, or a sequence of
        name -> weight dicts whose non-zero names are exactly the step's (`rescore_weights`); finite and not zero, negative is legal.
        Returns dict(winner [W] int64: local candidate indices, -1 where nothing is eligible; cost [W]: +inf there; totals [W][C]
        or None: every candidate's weighted cost, NaN without FX_FLAG_COSTED).  The bits are those of a plan step run with these
        weights.  It is the device selection only: nothing of the step is rewritten, and no host walk follows.
        pred [C] / resp [C] (fx_rescore_agent_rows): rows of a pass that ran beside the step -- pred in place
        of the step's prediction row, resp one more term, "responsibility", at its sorted place; the weights then follow
        `effective_cost_names`."""
        w, n, pred, resp = self._rescore_set(weights, agent, pred, resp)
        n_vec = w.shape[0]
        winner, cost = np.empty(n_vec, np.int64), np.empty(n_vec)
        tot = np.empty((n_vec, n)) if totals else None
        if pred is None and resp is None:
            check(lib().fx_rescore_agent(self._ctx, int(agent), n_vec, _ptr(w), _ptr(winner), _ptr(cost), _ptr(tot)))
        else:
            check(lib().fx_rescore_agent_rows(self._ctx, int(agent), n_vec, _ptr(w), _ptr(pred), _ptr(resp), _ptr(winner), _ptr(cost),
                                              _ptr(tot)))
        return dict(winner=winner, cost=cost, totals=tot)

    def rescore_batch(self, weights_per_agent, agents=None, pred=None, resp=None) -> list:
        """`rescore` for several agents of the context in ONE call (fx_rescore_batch): three launches at most
        and one copy each way whatever the number of agents, every agent's result the bits of its own call.  weights_per_agent: per
        listed agent what `rescore` takes; agents: their indices in any order (None: 0 .. len - 1); pred / resp: per listed agent
        a row [C] or None (None: no agent has one).  Returns one dict(winner [W_a], cost [W_a]) per listed agent."""
        n_agents = len(weights_per_agent)
        agents, ids = self._listed(agents, n_agents)
        pred = [None] * n_agents if pred is None else list(pred)
        resp = [None] * n_agents if resp is None else list(resp)
        if not (len(agents) == len(pred) == len(resp) == n_agents):
            raise ValueError(f"{n_agents} weight sets for {len(agents)} agents, {len(pred)} pred and {len(resp)} resp rows")
        if n_agents == 0:
            return []
        sets = [self._rescore_set(weights_per_agent[i], a, pred[i], resp[i]) for i, a in enumerate(agents)]
        n_vec = np.array([s[0].shape[0] for s in sets], np.int32)
        w = np.ascontiguousarray(np.concatenate([s[0].ravel() for s in sets]))
        total = int(n_vec.sum())
        winner, cost = np.empty(total, np.int64), np.empty(total)
        # (a table of the agents' rows, NULL for an agent without one; no agent has one: no table)
        table = lambda k: None if all(s[k] is None for s in sets) else (C.c_void_p * n_agents)(*[_ptr(s[k]) for s in sets])
        check(lib().fx_rescore_batch(self._ctx, n_agents, _ptr(ids), _ptr(n_vec), _ptr(w), table(2), table(3), _ptr(winner), _ptr(cost)))
        ends = np.cumsum(n_vec)
        return [dict(winner=winner[e - k:e], cost=cost[e - k:e]) for e, k in zip(ends, n_vec)]

    @property
    def last_rescore_ms(self) -> float:
        """device time of the last re-score's launches"""
        return float(lib().fx_last_rescore_ms(self._ctx))

    # -- the last step's obstacle stage under other prediction sets, on the device --
    def _hypothesis_shape(self, agent: int):
        """(K, P, candidates) of the agent's upload; zeros for an agent that is not there"""
        inp = self._agent_input(agent)
        return (int(inp.obstacles["K"]), int(inp.obstacles["P"]), inp.n_candidates) if inp is not None else (0, 0, 0)

    def hypotheses(self, prediction_sets, agent: int = 0, pred: bool = False, totals: bool = False, collisions: bool = False) -> dict:
        """The agent's last step under H other prediction sets in one call (fx_eval_hypotheses_agent): what a plan step with each of
        them would have selected, the walk not run again.  `prediction_sets`: a sequence of packed predictions
        (`problem.pack_predictions`, or `problem.hypothesis_arrays` of one); a set that has not the upload's K and P is padded
        with absent obstacles and re-strided by `hypothesis_arrays` (more obstacles than the upload: ValueError).
        Returns dict(winner [H] int64: local candidate indices, -1 where nothing is eligible; cost [H]: +inf there;
        n_collisions [H] int64; pred [H][C] / totals [H][C] / collisions [H][C] bool, each None unless asked for).  For a step
        whose obstacle stage ran as its own kernel the bits are those of a plan step with these predictions; for one that ran
        it inside the walk those of the same step forced to set_obstacle_stage(2, last_hypotheses_info["steps_per_item"]).  It
        is the device selection only: nothing of the step is rewritten, and no host walk follows."""
        sets = list(prediction_sets) if isinstance(prediction_sets, (list, tuple)) else [prediction_sets]
        n_hyp = len(sets)
        K, P, n = self._hypothesis_shape(agent)
        keep, hyp = [], (_abi.FxHypothesis * max(n_hyp, 1))()
        for h, s in enumerate(sets):
            _pack_hypothesis(hyp[h], s, K, P, keep)
        H = max(n_hyp, 1)
        r, out = _hypothesis_outputs(H, (H, n), pred, totals, collisions)
        check(lib().fx_eval_hypotheses_agent(self._ctx, int(agent), n_hyp, hyp, C.byref(out)))
        return dict(winner=r["winner"], cost=r["cost"], n_collisions=r["n_collisions"], pred=r["pred"], totals=r["total"],
                    collisions=None if r["collision"] is None else r["collision"].astype(bool))

    def hypotheses_batch(self, prediction_sets_per_agent, agents=None, pred: bool = False, totals: bool = False,
                         collisions: bool = False) -> list:
        """`hypotheses` for several agents of the context in ONE call (fx_eval_hypotheses_batch): three
        launches per round and one copy each way whatever the number of agents, every agent's result the bits of its own call.
        prediction_sets_per_agent: per listed agent what `hypotheses` takes, each agent's sets brought to that agent's K and P by
        `hypothesis_arrays` exactly as `hypotheses` does it; agents: their indices in any order (None: 0 .. len - 1).  Returns one
        dict per listed agent as `hypotheses` returns it (winner [H_a], cost [H_a], n_collisions [H_a], pred / totals /
        collisions [H_a][C_a] or None); the arrays are views of the call's concatenated ones.  It is the device selection only:
        nothing of the steps is rewritten, and no host walk follows."""
        per_agent = list(prediction_sets_per_agent)
        n_agents = len(per_agent)
        agents, ids = self._listed(agents, n_agents)
        if len(agents) != n_agents:
            raise ValueError(f"{n_agents} lists of prediction sets for {len(agents)} agents")
        if n_agents == 0:
            return []
        per_agent = [list(s) if isinstance(s, (list, tuple)) else [s] for s in per_agent]
        n_hyp = np.array([len(s) for s in per_agent], np.int32)
        pairs = int(n_hyp.sum())
        keep, hyp = [], (_abi.FxHypothesis * max(pairs, 1))()
        at, n_cand = 0, []
        for a, sets in zip(agents, per_agent):
            K, P, n = self._hypothesis_shape(a)
            n_cand.append(n)
            for s in sets:
                _pack_hypothesis(hyp[at], s, K, P, keep)
                at += 1
        cells = int(sum(int(h) * n for h, n in zip(n_hyp, n_cand)))
        r, out = _hypothesis_outputs(max(pairs, 1), cells, pred, totals, collisions)
        check(lib().fx_eval_hypotheses_batch(self._ctx, n_agents, _ptr(ids), _ptr(n_hyp), hyp, C.byref(out)))
        res, p0, c0 = [], 0, 0
        for h, n in zip((int(x) for x in n_hyp), n_cand):
            block = lambda a: None if a is None else a[c0:c0 + h * n].reshape(h, n)
            col = block(r["collision"])
            res.append(dict(winner=r["winner"][p0:p0 + h], cost=r["cost"][p0:p0 + h], n_collisions=r["n_collisions"][p0:p0 + h],
                            pred=block(r["pred"]), totals=block(r["total"]), collisions=None if col is None else col.view(np.bool_)))
            p0, c0 = p0 + h, c0 + h * n
        return res

    @property
    def last_hypotheses_ms(self) -> float:
        """device time of the last hypotheses call's launches"""
        return float(lib().fx_last_hypotheses_ms(self._ctx))

    @property
    def last_hypotheses_info(self) -> dict:
        """steps per item, rounds of hypotheses and kernel launches of the last hypotheses call"""
        return dict(zip(("steps_per_item", "rounds", "launches"), self._info3(lib().fx_last_hypotheses_info)))

    def costmap_view(self, agent: int = 0):
        """(device pointer of the agent's raw cost rows f64 [n_cost][ld], ld, n_cost) of a step that stored them (fx_device_costmap_view)"""
        p, ld, n_cost = C.c_void_p(), C.c_int64(0), C.c_int32(0)
        check(lib().fx_device_costmap_view(self._ctx, int(agent), C.byref(p), C.byref(ld), C.byref(n_cost)))
        return p.value, int(ld.value), int(n_cost.value)

    def plane(self, name_or_index, agent: int = 0) -> np.ndarray:
        """[S, C] one plane of every candidate."""
        inp = self._inputs[agent]
        p = _abi.PLANE_INDEX[name_or_index] if isinstance(name_or_index, str) else int(name_or_index)
        out = np.zeros((inp.n_samples, inp.n_candidates))
        check(lib().fx_read_plane_agent(self._ctx, agent, p, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def bundle(self, agent: int = 0) -> np.ndarray:
        """[C, 14, S] whole bundle (D2H of every plane; debugging / logging only)."""
        return np.ascontiguousarray(np.stack([self.plane(p, agent) for p in range(_abi.FX_NUM_PLANES)]).transpose(2, 0, 1))

    def set_risk_obstacles(self, tables: dict, agent: int = 0):
        """Obstacle tables of the trajectory risk (risk.obstacle_tables) for the next `risk` calls of this agent."""
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        t = {k: np.ascontiguousarray(v) for k, v in tables.items() if isinstance(v, np.ndarray)}
        self._risk_tables = t    # (kept alive for the call; the library copies them)
        self._risk_K = {**self._risk_K, agent: int(tables["K"])}   # (shape of risk_detail's columns)
        f = lambda n: t[n].ctypes.data_as(pd)
        i = lambda n: t[n].ctypes.data_as(pi)
        check(lib().fx_set_risk_obstacles_agent(self._ctx, agent, int(tables["K"]), int(tables["P"]), f("pos"), f("cov"), f("cov_inv"),
                                                f("yaw"), f("v"), i("n_pos"), i("n_yaw"), i("n_v"), f("length"), f("width"), f("mass"),
                                                i("cls")))

    def _risk_ids(self, ids, agent):
        """(rows of the result, n_ids and ids as the library takes them, the array behind ids) of a risk call: ids None is every
        candidate"""
        if ids is None:
            return self._inputs[agent].n_candidates, 0, None, None
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        return len(ids), len(ids), _ptr(ids, _PI64), ids

    def risk(self, params, ids=None, agent: int = 0):
        """(ego_risk, obst_risk, min_risk_index) of the last plan step's candidates on the device (fx_eval_risk_agent).
        ids None: every VALID & FEASIBLE & RETURNED candidate -- the arrays then have C entries, NaN for the others; the index is
        the arg-min of ego + obst (ties to the lower index), -1 when there is none."""
        pd = C.POINTER(C.c_double)
        n, n_ids, idp, ids = self._risk_ids(ids, agent)
        ego, obst = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        idx = C.c_int64(-1)
        check(lib().fx_eval_risk_agent(self._ctx, agent, C.byref(params), n_ids, idp, ego.ctypes.data_as(pd), obst.ctypes.data_as(pd),
                                       C.byref(idx)))
        return ego[:n], obst[:n], int(idx.value)

    def risk_batch(self, params, ids=None, agents=None) -> list:
        """`risk` of several agents of the last plan step in ONE call (fx_eval_risk_batch): per listed agent
        the (ego_risk, obst_risk, min_risk_index) that risk(params_a, ids_a, agent=a) returns, bit for bit; the arrays are views of
        the call's concatenated ones.  params: one FxRiskParams for all or one per listed agent; ids: None (no agent has a list) or
        per listed agent None (every candidate) or an int array; agents None: every agent of the last upload, in order; the
        obstacles are each agent's `set_risk_obstacles`."""
        listed, al = self._listed(agents)
        n = len(listed)
        params = _broadcast_params(params, _abi.FxRiskParams, n)
        ids, id_args, _alive = _id_tables(ids, n)
        if len(params) != n or len(ids) != n:
            raise ValueError(f"{len(params)} params and {len(ids)} id lists for {n} agents")
        prm = (_abi.FxRiskParams * max(n, 1))(*params)
        counts, off = self._row_counts(listed, ids)
        ego, obst = np.zeros(max(int(off[-1]), 1)), np.zeros(max(int(off[-1]), 1))
        idx = np.full(max(n, 1), -1, np.int64)
        out = _abi.FxRiskBatchOutputs(ego.ctypes.data, obst.ctypes.data, idx.ctypes.data)
        check(lib().fx_eval_risk_batch(self._ctx, n, _ptr(al, _PI32), prm, *id_args, C.byref(out)))
        return [(ego[off[i]:off[i + 1]], obst[off[i]:off[i + 1]], int(idx[i])) for i in range(n)]

    def set_reach_sets(self, tables: dict, agent: int = 0):
        """Reach-set tables (risk.reach_set_tables) for the reach-set responsibility of the next `risk_costs` calls of this
        agent.  Call it after set_risk_obstacles: the entries index that call's obstacles, and new obstacles clear them."""
        pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        t = {k: np.ascontiguousarray(tables[k], dtype=np.int32) for k in ("entry_obs", "entry_part_off", "part_step", "part_vert_off")}
        verts = np.ascontiguousarray(tables["verts"], dtype=np.float64).reshape(-1, 2)
        i = lambda n: t[n].ctypes.data_as(pi)
        check(lib().fx_set_reach_sets_agent(self._ctx, agent, len(t["entry_obs"]), i("entry_obs"), i("entry_part_off"), len(t["part_step"]),
                                            i("part_step"), i("part_vert_off"), len(verts), verts.ctypes.data_as(pd)))

    def _risk_costs(self, params, cost_params, ids, agent):
        K = self._risk_K.get(agent, 0)
        n, n_ids, idp, ids = self._risk_ids(ids, agent)
        _check_risk_cost_lengths(cost_params, n, K)
        res = {k: np.zeros(max(n, 1)) for k in _RISK_ROWS + (_RISK_COST_ROWS if cost_params is not None else [])}
        res.update({k: np.zeros((K, max(n, 1))) for k in _RISK_COLS})
        idx = np.full(2, -1, np.int64)
        out = _bind(_abi.FxRiskOutputs(), dict(res, min_risk_index=idx[:1], min_cost_index=idx[1:]))
        if n > 0:   # (an empty id list: nothing to evaluate, no arg-min)
            check(lib().fx_eval_risk_costs_agent(self._ctx, agent, C.byref(params), C.byref(cost_params) if cost_params is not None else None,
                                                 n_ids, idp, C.byref(out)))
        res = {k: (a[:, :n].T if k in _RISK_COLS else a[:n]) for k, a in res.items()}   # [n, K] views of the obstacle-major columns
        res["min_risk_index"] = int(idx[0])
        if cost_params is not None:
            res["min_cost_index"] = int(idx[1])
        return res

    def risk_detail(self, params, ids=None, agent: int = 0) -> dict:
        """calc_risk's seven results of the last plan step's candidates on the device (fx_eval_risk_costs_agent, DESIGN.md section
        13): ego_risk, obst_risk (bit for bit what `risk` returns), obst_harm_occ [n]; ego_risk_max, obst_risk_max, ego_harm_max,
        obst_harm_max [n, K] (columns in the order of the obstacle tables' keys); min_risk_index.  ids as in `risk`."""
        return self._risk_costs(params, None, ids, agent)

    def risk_costs(self, params, cost_params, ids=None, agent: int = 0) -> dict:
        """risk_detail plus the risk-cost principles of risk.risk_cost_params: bayes, equality, maximin, ego, responsibility, their
        weighted total, the boundary_harm they used [n], and min_cost_index, the arg-min of the total (ties to the lower index, NaN
        skipped, -1 when nothing is left)."""
        return self._risk_costs(params, cost_params, ids, agent)

    def _risk_costs_batch(self, params, cost_params, ids, agents) -> list:
        listed, al = self._listed(agents)
        n = len(listed)
        params = _broadcast_params(params, _abi.FxRiskParams, n)
        costs = [None] * n if cost_params is None else _broadcast_params(cost_params, _abi.FxRiskCostParams, n)
        ids, id_args, _alive = _id_tables(ids, n)
        if len(params) != n or len(ids) != n or len(costs) != n:
            raise ValueError(f"{len(params)} params, {len(costs)} cost params and {len(ids)} id lists for {n} agents")
        counts, off = self._row_counts(listed, ids)
        Ks = [self._risk_K.get(a, 0) for a in listed]
        for a, m, K, cp in zip(listed, counts, Ks, costs):
            _check_risk_cost_lengths(cp, m, K, f"agent {a}: ")
        prm = (_abi.FxRiskParams * max(n, 1))(*params)
        pcp = C.POINTER(_abi.FxRiskCostParams)
        cpp = (pcp * max(n, 1))(*[C.cast(None, pcp) if cp is None else C.pointer(cp) for cp in costs])
        coff = np.concatenate([[0], np.cumsum([K * m for K, m in zip(Ks, counts)])]).astype(np.int64)
        any_cost = any(cp is not None for cp in costs)
        flat = {k: np.zeros(max(int(off[-1]), 1)) for k in _RISK_ROWS + (_RISK_COST_ROWS if any_cost else [])}
        flat.update({k: np.zeros(max(int(coff[-1]), 1)) for k in _RISK_COLS})
        idx = np.full((2, max(n, 1)), -1, np.int64)
        out = _bind(_abi.FxRiskCostBatchOutputs(), dict(flat, min_risk_index=idx[0], min_cost_index=idx[1]))
        check(lib().fx_eval_risk_costs_batch(self._ctx, n, _ptr(al, _PI32), prm, cpp if any_cost else None, *id_args, C.byref(out)))
        res = []
        for i in range(n):
            m, K = counts[i], Ks[i]
            d = {k: flat[k][off[i]:off[i + 1]] for k in _RISK_ROWS + (_RISK_COST_ROWS if costs[i] is not None else [])}
            d.update({k: flat[k][coff[i]:coff[i + 1]].reshape(K, m).T for k in _RISK_COLS})   # [n, K] views of the obstacle-major columns
            d["min_risk_index"] = int(idx[0, i])
            if costs[i] is not None:
                d["min_cost_index"] = int(idx[1, i])
            res.append(d)
        return res

    def risk_detail_batch(self, params, ids=None, agents=None) -> list:
        """`risk_detail` of several agents of the last plan step in ONE call (fx_eval_risk_costs_batch): per
        listed agent the dict risk_detail(params_a, ids_a, agent=a) returns, bit for bit; the arrays and the [n, K] column views
        are views of the call's concatenated ones.  params, ids, agents as in `risk_batch`."""
        return self._risk_costs_batch(params, None, ids, agents)

    def risk_costs_batch(self, params, cost_params, ids=None, agents=None) -> list:
        """`risk_costs` of several agents of the last plan step in ONE call (fx_eval_risk_costs_batch): per
        listed agent the dict risk_costs(params_a, cost_params_a, ids_a, agent=a) returns, bit for bit.  cost_params: one
        FxRiskCostParams for all or one per listed agent, None for an agent that gets the detail alone; params, ids, agents as in
        `risk_batch`; obstacles and reach sets are each agent's `set_risk_obstacles` / `set_reach_sets`."""
        return self._risk_costs_batch(params, cost_params, ids, agents)

    @property
    def last_risk_costs_batch_rounds(self) -> int:
        """rounds of scratch the last `risk_detail_batch` / `risk_costs_batch` call took (-1 before the first)"""
        return int(lib().fx_last_risk_costs_batch_rounds(self._ctx))

    @property
    def last_risk_ms(self) -> float:
        """device time of the last `risk` / `risk_batch` / `risk_detail` / `risk_costs` / `risk_detail_batch` / `risk_costs_batch` /
        `responsibility_cost` / `responsibility_cost_batch` call (its kernels)"""
        return float(lib().fx_last_risk_ms(self._ctx))

    # -- the responsibility cost as a weighted term --
    def responsibility_cost(self, params, cost_params, weight: float, ids=None, agent: int = 0, prediction: str = "step") -> dict:
        """The `responsibility` cost term (partial_cost_functions.py:359-387) for candidates of the last plan step, on the device
        (fx_eval_responsibility_cost_agent): resp [n], get_responsibility_cost over calc_risk's obst_risk_max in the mode of
        cost_params (risk.risk_cost_params with responsibility= the [K] vector or "reach_set"; nothing else of it is read);
        total [n], the step's weighted cost re-summed from its raw cost rows with weight * resp at its place in the name-sorted
        list; ego_risk, obst_risk [n] as `risk` returns them; best_index / best_cost as `prediction_probability`; prediction, the
        [n] entry summed instead of the step's own (None with "step").  ids None: every
        candidate, NaN rows for the ones without a cost.  prediction "probability": the prediction entry of the re-sum is the
        prob of `prediction_probability` (ego length and width of params) over the same candidates instead of the step's own.
        Needs write_costmap, and the bundle or ids inside the agent's sparse set.  Nothing the step wrote is touched."""
        if prediction not in ("step", "probability"):
            raise ValueError(f"prediction {prediction!r}: 'step' or 'probability'")
        _check_responsibility(cost_params, weight, self._risk_K.get(agent, 0))
        pred = None
        if prediction == "probability":
            pred = np.ascontiguousarray(self.prediction_probability(params.ego_length, params.ego_width, ids=ids, agent=agent)["prob"])
        n, n_ids, idp, ids = self._risk_ids(ids, agent)
        rp = _resp_cost_params(cost_params, weight, pred)
        res = {k: np.zeros(max(n, 1)) for k in _RESP_ROWS}
        best_index, best_cost = np.full(1, -1, np.int64), np.full(1, np.nan)
        out = _bind(_abi.FxRespCostOutputs(), dict(res, best_index=best_index, best_cost=best_cost))
        if n > 0 or ids is None:   # (an empty id list: nothing to evaluate, no arg-min)
            check(lib().fx_eval_responsibility_cost_agent(self._ctx, int(agent), C.byref(params), C.byref(rp), n_ids, idp, C.byref(out)))
        res = {k: a[:n] for k, a in res.items()}
        res["best_index"], res["best_cost"] = int(best_index[0]), float(best_cost[0])
        res["prediction"] = pred   # (the prediction entry that was summed instead of the step's own, or None)
        return res

    def responsibility_cost_batch(self, params, cost_params, weights, agents=None, prediction: str = "step") -> list:
        """`responsibility_cost` over every candidate of several agents of the last plan step in ONE call
        (fx_eval_responsibility_cost_batch): per listed agent the dict responsibility_cost(agent=a) returns,
        bit for bit -- resp, total, ego_risk, obst_risk [C of that agent] as views of the call's concatenated arrays, best_index,
        best_cost, prediction.  params, cost_params, weights: one per listed agent; agents None: every agent of the last upload,
        in order; obstacles and reach sets are each agent's `set_risk_obstacles` / `set_reach_sets`.  prediction "probability":
        ONE `prediction_probability_batch` over the same agents first (ego length and width of each params), each agent's prob
        as its prediction entry; a sequence of the two words, one per listed agent: that call over the "probability" ones."""
        listed, al = self._listed(agents)
        n = len(listed)
        kinds = [prediction] * n if isinstance(prediction, str) else list(prediction)
        if len(kinds) != n or any(k not in ("step", "probability") for k in kinds):
            raise ValueError(f"prediction {prediction!r}: 'step' or 'probability', or one of them per listed agent")
        params, cost_params, weights = list(params), list(cost_params), [float(w) for w in weights]
        if not (len(params) == len(cost_params) == len(weights) == n):
            raise ValueError(f"{len(params)} params, {len(cost_params)} cost_params and {len(weights)} weights for {n} agents")
        for a, cp, w in zip(listed, cost_params, weights):   # (the refusals of responsibility_cost, before any call)
            _check_responsibility(cp, w, self._risk_K.get(a, 0), f"agent {a}: ")
        preds = [None] * n
        js = [i for i in range(n) if kinds[i] == "probability"]
        if js:
            pp = self.prediction_probability_batch([params[i].ego_length for i in js], [params[i].ego_width for i in js],
                                                   agents=[listed[i] for i in js])
            for i, r in zip(js, pp):
                preds[i] = np.ascontiguousarray(r["prob"])
        prm = (_abi.FxRiskParams * max(n, 1))(*params)
        rps = (_abi.FxRespCostParams * max(n, 1))(*[_resp_cost_params(cp, w, p) for cp, w, p in zip(cost_params, weights, preds)])
        counts, off = self._row_counts(listed)
        res = {k: np.zeros(max(int(off[-1]), 1)) for k in _RESP_ROWS}
        best_index, best_cost = np.full(max(n, 1), -1, np.int64), np.full(max(n, 1), np.nan)
        out = _bind(_abi.FxRespCostBatchOutputs(), dict(res, best_index=best_index, best_cost=best_cost))
        check(lib().fx_eval_responsibility_cost_batch(self._ctx, n, _ptr(al, _PI32), prm, rps, C.byref(out)))
        return [dict({k: a[off[i]:off[i + 1]] for k, a in res.items()}, best_index=int(best_index[i]), best_cost=float(best_cost[i]),
                     prediction=preds[i]) for i in range(n)]

    # -- collision probability as the prediction cost --
    def prediction_probability(self, ego_length: float, ego_width: float, ids=None, agent: int = 0, per_obstacle: bool = False,
                               source: str = "probability") -> dict:
        """The `prediction` cost of the reference's C++ route (cf.CalculateCollisionProbabilityFast) for candidates of the last plan
        step, on the device (fx_eval_prediction_prob_agent): prob [n], the sum over the obstacles of `set_risk_obstacles` -- in
        their order -- of the summed get_collision_probability_fast; total [n], the step's weighted cost re-summed from its raw cost
        rows with prob in the prediction entry; best_index / best_cost, the (total, index) minimum over the selectable
        collision-free candidates (-1 / NaN when there is none); per_obstacle: prob_obs [n, K].  ids None: every candidate, NaN
        rows for the ones without a cost.  source "step" re-sums with the step's own prediction entry instead (no probability is
        evaluated): its total is the step's cost bit for bit.  Needs write_costmap and a cost list with a prediction term, and the
        bundle or ids inside the agent's sparse set (`materialise`).  Nothing the step wrote is touched."""
        if source not in _abi.PRED_SOURCES:
            raise ValueError(f"source {source!r}: one of {sorted(_abi.PRED_SOURCES)}")
        n, n_ids, idp, ids = self._risk_ids(ids, agent)
        params = _abi.FxPredProbParams(float(ego_length), float(ego_width), _abi.PRED_SOURCES[source])
        res = dict(prob=np.zeros(max(n, 1)), total=np.zeros(max(n, 1)))
        if per_obstacle:
            res["prob_obs"] = np.zeros((self._risk_K.get(agent, 0), max(n, 1)))
        best_index, best_cost = np.full(1, -1, np.int64), np.full(1, np.nan)
        out = _bind(_abi.FxPredProbOutputs(), dict(res, best_index=best_index, best_cost=best_cost))
        if n > 0 or ids is None:   # (an empty id list: nothing to evaluate, no arg-min)
            check(lib().fx_eval_prediction_prob_agent(self._ctx, int(agent), C.byref(params), n_ids, idp, C.byref(out)))
        res = {k: (a[:, :n].T if k == "prob_obs" else a[:n]) for k, a in res.items()}
        res["best_index"], res["best_cost"] = int(best_index[0]), float(best_cost[0])
        return res

    def prediction_probability_batch(self, ego_lengths, ego_widths, agents=None, source: str = "probability") -> list:
        """`prediction_probability` over every candidate of several agents of the last plan step in ONE call
        (fx_eval_prediction_prob_batch): per listed agent a dict of prob, total [C of that agent], best_index
        and best_cost, bit for bit what prediction_probability(agent=a) returns.  ego_lengths / ego_widths: one number for all or
        one per listed agent; agents None: every agent of the last upload, in order; the obstacles are each agent's
        `set_risk_obstacles`.  The arrays are views of the call's concatenated ones."""
        if source not in _abi.PRED_SOURCES:
            raise ValueError(f"source {source!r}: one of {sorted(_abi.PRED_SOURCES)}")
        listed, al = self._listed(agents)
        n = len(listed)
        ln, wd = np.broadcast_to(np.asarray(ego_lengths, np.float64), (n,)), np.broadcast_to(np.asarray(ego_widths, np.float64), (n,))
        params = (_abi.FxPredProbParams * max(n, 1))(*[_abi.FxPredProbParams(float(ln[i]), float(wd[i]), _abi.PRED_SOURCES[source])
                                                       for i in range(n)])
        counts, off = self._row_counts(listed)
        prob, total = np.zeros(max(int(off[-1]), 1)), np.zeros(max(int(off[-1]), 1))
        best_index, best_cost = np.full(max(n, 1), -1, np.int64), np.full(max(n, 1), np.nan)
        out = _abi.FxPredProbBatchOutputs(prob.ctypes.data, total.ctypes.data, best_index.ctypes.data, best_cost.ctypes.data)
        check(lib().fx_eval_prediction_prob_batch(self._ctx, n, _ptr(al, _PI32), params, C.byref(out)))
        return [dict(prob=prob[off[i]:off[i + 1]], total=total[off[i]:off[i + 1]], best_index=int(best_index[i]),
                     best_cost=float(best_cost[i])) for i in range(n)]

    @property
    def last_predprob_ms(self) -> float:
        """device time of the last `prediction_probability` / `prediction_probability_batch` call (its kernels); -1 before the first"""
        return float(lib().fx_last_predprob_ms(self._ctx))

    def topk(self, k: int):
        n = len(self._inputs)
        cost = np.zeros((n, k))
        idx = np.zeros((n, k), np.int64)
        check(lib().fx_read_topk_batch(self._ctx, int(k), cost.ctypes.data_as(C.POINTER(C.c_double)),
                                       idx.ctypes.data_as(C.POINTER(C.c_int64))))
        return cost, idx

    def topk_to_device(self, k: int, d_cost_ptr: int, d_index_ptr: int):
        check(lib().fx_topk_to_device(self._ctx, int(k), C.c_void_p(d_cost_ptr), C.c_void_p(d_index_ptr)))

    @property
    def device_bytes(self) -> int:
        return int(lib().fx_device_bytes(self._ctx))

    @property
    def last_kernel_ms(self) -> float:
        return float(lib().fx_last_kernel_ms(self._ctx))

    @property
    def last_eval_kernel_ms(self) -> float:
        return float(lib().fx_last_eval_kernel_ms(self._ctx))
