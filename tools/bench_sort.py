#!/usr/bin/env python3
"""The cost order of all candidates: sorted on the device and read by rank against today's host path,
fx_read_costs plus the NumPy expressions of PlanStepResult.sorted_ids, measured in the same process.  One JSON line per size.

  config1   5 x 9 x 13 (+ d0) = 630 candidates, 5 obstacles          (the planner's operating point: one workgroup, one launch)
  config3   19 x 51 x 51 (+ d0) = 50 388 candidates, 20 obstacles
  config5   32 agents x 39 x 51 x 51 (+ d0) = 32 x 103 428 candidates (one batched sort, agents are grid.y)
  1m        19 x 230 x 229 (+ d0) = 1 005 100 candidates

--grid T,V,D measures one grid of T x V x (D + 1) candidates with 5 obstacles instead (the sweep for the size at which
PlanStepResult.ranked_ids switches from the host's sort to the device's).  Without --size every size runs in a process of its own.  Per size, after --warmup repetitions, the median and p5 / p95 of --reps:
  device_sort          device time of the sort alone (events around its launches)
  sort_ranked64_wall   host clock around sort_candidates + ranked(0, 64)         (every agent of a batch)
  sort_all_wall        host clock around sort_candidates + the whole order read back
  host_wall            host clock around costs() + np.nonzero + np.argsort(kind="stable")
The pool is FX_FLAG_COSTED, the steps are select-only (cost and flag planes are all a sort reads)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ("config1", "config3", "config5", "1m")


def stats(xs_ms):
    xs = np.asarray(xs_ms, float) * 1e3
    return dict(p50_us=float(np.median(xs)), p5_us=float(np.percentile(xs, 5)), p95_us=float(np.percentile(xs, 95)), reps=len(xs))


def run(size, reps, warmup, grid=None):
    from frenetix_motion_planner_amd import _abi, synthetic
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    kw = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, write_bundle=False, write_costmap=False)
    if grid is not None:
        inps = [synthetic.make_inputs(grid=grid, n_obstacles=5, lead_gap=25.0, **kw)]
    elif size == "config5":
        inps = synthetic.stress_agents(32, grid=(39, 51, 51), hull_builder=build_obstacle_hulls, write_bundle=False)   # (no cost map either)
    else:
        grid, n_obst = dict(config1=((5, 9, 13), 5), config3=((19, 51, 51), 20))[size] if size != "1m" else ((19, 230, 229), 20)
        inps = [synthetic.make_inputs(grid=grid, n_obstacles=n_obst, lead_gap=25.0, **kw)]
    A, C = len(inps), inps[0].n_candidates
    bit = _abi.FX_FLAG_COSTED
    with FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in inps), max_steps=inps[0].N, max_agents=A, max_obstacles=32,
                      max_pred_steps=64) as eng:
        eng.plan_batch(inps) if A > 1 else eng.plan_step(inps[0])

        def sort():
            return eng.sort_candidates_batch(bit, 0)[0] if A > 1 else [eng.sort_candidates(0, bit, 0)[0]]

        def host():
            out = []
            for a in range(A):
                cost, flags = eng.costs(a)
                ids = np.nonzero((flags & bit) != 0)[0]
                out.append(ids[np.argsort(cost[ids], kind="stable")])
            return out

        dev, w64, wall, whost = [], [], [], []
        for r in range(reps + warmup):
            t0 = time.perf_counter()
            n_pool = sort()
            first = [eng.ranked(0, min(64, int(n_pool[a])), a) for a in range(A)]
            t1 = time.perf_counter()
            n_pool = sort()
            d = eng.last_sort_ms
            t2 = time.perf_counter()
            n_pool = sort()
            order = [eng.ranked(0, int(n_pool[a]), a) for a in range(A)]
            t3 = time.perf_counter()
            want = host()
            t4 = time.perf_counter()
            if r == 0:
                assert all(np.array_equal(order[a], want[a]) and np.array_equal(first[a], want[a][:64]) for a in range(A))
            if r >= warmup:
                dev.append(d); w64.append((t1 - t0) * 1e3); wall.append((t3 - t2) * 1e3); whost.append((t4 - t3) * 1e3)
        print(json.dumps(dict(metric="sort", size=size, agents=A, candidates=C, pool=[int(x) for x in n_pool][:4], device_sort=stats(dev),
                              sort_ranked64_wall=stats(w64), sort_all_wall=stats(wall), host_wall=stats(whost))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=SIZES)
    ap.add_argument("--grid", help="T,V,D: one grid of T x V x (D + 1) candidates instead of a named size")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.grid:
        grid = tuple(int(x) for x in a.grid.split(","))
        return run("grid_%dx%dx%d" % grid, a.reps, a.warmup, grid)
    if a.size:
        return run(a.size, a.reps, a.warmup)
    for size in SIZES:   # one process per size
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--size", size, "--reps", str(a.reps), "--warmup", str(a.warmup)]).returncode
        if rc:
            sys.exit(rc)


if __name__ == "__main__":
    main()
