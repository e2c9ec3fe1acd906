#!/usr/bin/env python3
"""Select-only step + materialised survivors against the bundle-mode step.  One JSON line per row.

Device times are medians over --reps repetitions after --warmup: the step's from the events attached to its kernels
(set_timing("kernel"), last_kernel_ms), the list kernel's from the events attached to it (last_materialise_ms).  "wall" rows are
the host clock around the calls that end in a stream synchronise (what a planner waits for).

  config3   19 x 51 x 51 grid (+ d0), 20 obstacles:  bundle step | select-only step | select-only + materialise(winner + top-k)
            + read-back for k = 32, 64 and 800 (top-k beyond 64: the k cheapest selectable candidates taken from costs())
  1m        19 x 230 x 229 grid, 20 obstacles: the same three rows at k = 64
  --trace-workload: 20 materialise calls per k of config 3 and nothing else, for
      rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_materialise.py --trace-workload
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frenetix_motion_planner_amd import _abi, synthetic  # noqa: E402
from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls  # noqa: E402

WORK = dict(config3=dict(grid=(19, 51, 51), n_obstacles=20, lead_gap=25.0), north_star_1m=dict(grid=(19, 230, 229), n_obstacles=20, lead_gap=25.0))


def med(xs):
    xs = np.asarray(xs, float) * 1e3
    return dict(p50_us=float(np.median(xs)), p5_us=float(np.percentile(xs, 5)), p95_us=float(np.percentile(xs, 95)), reps=len(xs))


def survivors(eng, res, k):
    """the winner and the k cheapest selectable collision-free candidates"""
    if k <= 64:
        idx = eng.topk(k)[1][0]
    else:
        cost, flags = eng.costs()
        ok = np.nonzero(((flags & _abi.FX_FLAG_SELECTABLE) != 0) & ((flags & (_abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY)) == 0))[0]
        idx = ok[np.argsort(cost[ok], kind="stable")][:k]
    return np.unique(np.concatenate([[res["best_index"]], idx[idx >= 0]]).astype(np.int64))


def step_rows(name, kw, ks, reps, warmup):
    bundle = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, **kw)
    select = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, write_bundle=False, write_costmap=False, **kw)
    with FrenetEngine(max_candidates=bundle.n_candidates + 64, max_steps=bundle.N) as eng:
        eng.set_timing("kernel")
        for label, inp in (("bundle_step", bundle), ("select_only_step", select)):
            eng.upload(inp)
            dev, wall = [], []
            for r in range(reps + warmup):
                t0 = time.perf_counter()
                eng.evaluate()
                res = eng.finish()[0]
                t1 = time.perf_counter()
                if r >= warmup:
                    dev.append(eng.last_kernel_ms)
                    wall.append((t1 - t0) * 1e3)
            print(json.dumps(dict(metric=label, workload=name, candidates=inp.n_candidates, device=med(dev), wall=med(wall))), flush=True)
        for k in ks:
            ids = survivors(eng, res, k)
            dev, step, wall_m, wall_all = [], [], [], []
            for r in range(reps + warmup):
                t0 = time.perf_counter()
                eng.evaluate()
                res = eng.finish()[0]
                t1 = time.perf_counter()
                eng.materialise(ids)
                t2 = time.perf_counter()
                if r >= warmup:
                    dev.append(eng.last_materialise_ms)
                    step.append(eng.last_kernel_ms)
                    wall_m.append((t2 - t1) * 1e3)
                    wall_all.append((t2 - t0) * 1e3)
            d, s = med(dev), med(step)
            print(json.dumps(dict(metric="select_only_plus_materialise", workload=name, k=k, n=len(ids), list_kernel=d, step_device=s,
                                  device_sum_p50_us=d["p50_us"] + s["p50_us"], materialise_and_read_wall=med(wall_m),
                                  step_materialise_read_wall=med(wall_all))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-1m", action="store_true")
    ap.add_argument("--trace-workload", action="store_true")
    a = ap.parse_args()
    if a.trace_workload:
        kw = WORK["config3"]
        select = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, write_bundle=False, write_costmap=False, **kw)
        with FrenetEngine(max_candidates=select.n_candidates + 64, max_steps=select.N) as eng:
            res = eng.plan_step(select)
            for k in (32, 64, 800):
                ids = survivors(eng, res, k)
                for _ in range(20):
                    eng.materialise(ids)
        return
    step_rows("config3", WORK["config3"], (32, 64, 800), a.reps, a.warmup)
    if not a.skip_1m:
        step_rows("north_star_1m", WORK["north_star_1m"], (64,), a.reps, a.warmup)


if __name__ == "__main__":
    main()
