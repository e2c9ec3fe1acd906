"""Risk pass + arg-min (fx_risk_kernel.h) at the BASELINE config-3 size: 50 388 candidates, 20 obstacles
placed along candidates so that all of them are in range of many candidates.  Prints one JSON line: device-event time of the
risk call (median over --reps), gated (candidate, obstacle, step) triples and BVN evaluations, bytes read and an FP64
operation estimate with their shares of the MI355X peaks (8 TB/s HBM, 78.6 TFLOP/s FP64 vector, public specifications), and
the reference calc_risk's CPU time per trajectory recorded by tests/golden/gen_risk_golden.py.

--costs adds the per-obstacle detail pass and the risk-cost pass on the same step: device-event time of
risk_detail (detail kernel + arg-min) and of risk_costs (detail, both arg-mins and the cost kernel, reach-set responsibility
over six obstacles' polygons); the cost pass is their difference.

--wall instead measures the host side, which at planner size the kernels no longer hide: wall-clock time around risk() and
risk_costs() on an id list at grid (8, 16, 16) with 8 obstacles, after one warm-up call each, median over --reps.

Kernel time by rocprofv3, in a run of its own:  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_risk.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frenetix_motion_planner_amd import synthetic, risk  # noqa: E402
from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls  # noqa: E402
from tests.test_risk_gpu import _predictions, HARM, BASE, EGO  # noqa: E402

# FP64 operations of one BVN evaluation, counted from the kernel's expressions (exp ~ 20, erfc ~ 30 operations):
# low-|rho| branch 2 ng nodes x (7 + exp) + 2 Phi + 6; the other branches are of the same order
def bvn_ops(ng):
    return 2 * ng * (7 + 20) + 2 * 30 + 6


def wall(reps):
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(8, 16, 16), n_obstacles=4)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        _, flags = eng.costs()
        planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(7), n_obs=8)
        eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
        params = risk.risk_params(dict(BASE), HARM, **EGO)
        ids = np.nonzero((flags & 0xB) == 0xB)[0]
        cp = risk.risk_cost_params([1.0, 0.5, 2.0, 0.25, 1.5], boundary_harm="step", harm_coeff=(-4.591, 0.185))
        out = dict(metric="wall time of the risk calls, grid (8, 16, 16), 8 obstacles", candidates=inp.n_candidates, listed=int(len(ids)),
                   reps=reps)
        for name, call in (("risk", lambda: eng.risk(params, ids)), ("risk_costs", lambda: eng.risk_costs(params, cp, ids))):
            call()                             # allocation, first launch
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t0) * 1e3)
            out.update({f"{name}_wall_ms_median": float(np.median(ms)), f"{name}_wall_ms_min": float(np.min(ms)),
                        f"{name}_wall_ms_max": float(np.max(ms)), f"{name}_device_ms": eng.last_risk_ms})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--variant", default="log_reg_reduced_sym")
    ap.add_argument("--costs", action="store_true", help="also time risk_detail and risk_costs (DESIGN.md section 13)")
    ap.add_argument("--wall", action="store_true", help="wall-clock time of risk() and risk_costs() at planner size instead")
    a = ap.parse_args()
    if a.wall:
        return wall(a.reps)
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(19, 51, 51), n_obstacles=20)
    modes = dict(BASE)
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        _, flags = eng.costs()
        planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(3), n_obs=20)
        tabs = risk.obstacle_tables(preds, typ)
        risk.check_obstacle_classes(modes, tabs["classes"])
        eng.set_risk_obstacles(tabs)
        params = risk.risk_params(modes, HARM, **EGO)
        eng.risk(params)                       # allocation, first launch
        ms = []
        for _ in range(a.reps):
            eng.risk(params)
            ms.append(eng.last_risk_ms)
        extra = {}
        if a.costs:
            ids_ = np.nonzero((flags & 0xB) == 0xB)[0]
            keys = list(preds)
            sets = {}
            for n_, oid in enumerate(keys[:6]):   # polygons on the candidates' own points, growing with time
                parts = []
                for t_ in (0.3, 0.5, 1.0, 1.6, 2.2, 2.9):
                    st = int(np.array(t_ / inp.dt - 1, dtype=int))
                    c = np.array([np.median(planes["x"][ids_, st]), np.median(planes["y"][ids_, st])])
                    ang = 0.2 * n_ + 2 * np.pi * np.arange(5 + n_) / (5 + n_)
                    parts.append({t_: c + (1.0 + 0.8 * t_) * np.stack([np.cos(ang), np.sin(ang)], axis=1)})
                sets[oid] = parts
            eng.set_reach_sets(risk.reach_set_tables(sets, keys, inp.dt, inp.n_samples))
            cp = risk.risk_cost_params([1.0, 0.5, 2.0, 0.25, 1.5], boundary_harm="step", harm_coeff=(-4.591, 0.185), responsibility="reach_set")
            eng.risk_costs(params, cp)             # allocation, first launch
            md, mc = [], []
            for _ in range(a.reps):
                eng.risk_detail(params)
                md.append(eng.last_risk_ms)
                out_c = eng.risk_costs(params, cp)
                mc.append(eng.last_risk_ms)
            extra = dict(detail_ms_median=float(np.median(md)), detail_ms_min=float(np.min(md)), detail_ms_max=float(np.max(md)),
                         costs_ms_median=float(np.median(mc)), costs_ms_min=float(np.min(mc)), costs_ms_max=float(np.max(mc)),
                         cost_pass_ms=float(np.median(mc) - np.median(md)), min_cost_index=out_c["min_cost_index"],
                         reach_set_parts=sum(len(v) for v in sets.values()), device_bytes=eng.device_bytes)
    ids = np.nonzero((flags & 0xB) == 0xB)[0]
    S = planes["x"].shape[1]
    # gated triples, from the same means the kernel uses
    gated, ops = 0, 0
    x, y = planes["x"][ids], planes["y"][ids]
    for p in preds.values():
        pos, yaw, ln = p["pos_list"], p["orientation_list"], p["shape"]["length"]
        cov = p["cov_list"]
        for i in range(1, min(S, len(pos))):
            dev = np.array([np.cos(yaw[i]), np.sin(yaw[i])]) * ln / 2
            d = np.min([np.hypot(m[0] - x[:, i], m[1] - y[:, i]) for m in (pos[i - 1], pos[i - 1] + dev, pos[i - 1] - dev)], axis=0)
            g = int(np.count_nonzero(~(d > 5.0)))
            c = cov[i - 1] if np.any(cov[i - 1] != 0) else np.eye(2) * 0.1
            r = abs(c[1, 0] / np.sqrt(c[0, 0] * c[1, 1]))
            gated += g
            ops += g * 36 * bvn_ops(3 if r < 0.3 else (6 if r < 0.75 else 10))
    n = len(planes["x"])
    bytes_read = 4 * S * n * 8 + n * 4 + 2 * n * 8   # x, y, theta, v planes + flags + risk outputs
    t = float(np.median(ms)) * 1e-3
    g = np.load(os.path.join(ROOT, "tests", "golden", "risk_config3_obs20.npz"))
    out = dict(metric="risk pass + arg-min, config 3", ms_max=float(np.max(ms)), candidates=n, selected=int(len(ids)), obstacles=len(preds), steps=S,
               ms_median=float(np.median(ms)), ms_min=float(np.min(ms)), gated_triples=gated, bvn_evaluations=36 * gated,
               bytes_read=bytes_read, hbm_share=bytes_read / t / 8.0e12, fp64_ops_estimate=ops,
               fp64_share=ops / t / 78.6e12, us_per_candidate=t * 1e6 / max(len(ids), 1),
               reference_cpu_ms_per_trajectory=float(g["ref_seconds_per_trajectory"]) * 1e3)
    out.update(extra)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
