#!/usr/bin/env python3
"""Select-only step + materialised survivors against the bundle-mode step.  One JSON line per row.

Device times are medians over --reps repetitions after --warmup: the step's from the events attached to its kernels
(set_timing("kernel"), last_kernel_ms), the list kernel's from the events attached to it (last_materialise_ms).  "wall" rows are
the host clock around the calls that end in a stream synchronise (what a planner waits for).

  config3   19 x 51 x 51 grid (+ d0), 20 obstacles:  bundle step | select-only step | select-only + materialise(winner + top-k)
            + read-back for k = 32, 64 and 800 (top-k beyond 64: the k cheapest selectable candidates taken from costs())
  1m        19 x 230 x 229 grid, 20 obstacles: the same three rows at k = 64
  --lanes-batch, legs alternating in one process, medians of --reps after --warmup:
      list kernel at 1, 8 and 32 lanes per candidate: config 3 at k = 32, 64 and 800, the 1 M grid at k = 64
      one materialise_batch against the loop of per-agent materialise calls, at 1, 8 and 32 lanes, each agent's winner + top-32:
      32 agents x 630 candidates with 5 obstacles, and 5 agents x 10 488 candidates (BASELINE config 4's shape)
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


LANES = (1, 8, 32)
BATCHES = dict(agents32_630=dict(n_agents=32, grid=(5, 9, 13), n_obstacles=5), config4_5x10488=dict(n_agents=5, grid=(19, 23, 23), n_obstacles=5))


def lanes_rows(name, kw, ks, reps, warmup):
    """the list kernel of one agent at 1, 8 and 32 lanes per candidate, the legs alternating"""
    select = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, write_bundle=False, write_costmap=False, **kw)
    with FrenetEngine(max_candidates=select.n_candidates + 64, max_steps=select.N) as eng:
        res = eng.plan_step(select)
        for k in ks:
            ids = survivors(eng, res, k)
            dev, wall = {g: [] for g in LANES}, {g: [] for g in LANES}
            for r in range(reps + warmup):
                for g in LANES:
                    eng.set_materialise_lanes(g)
                    t0 = time.perf_counter()
                    eng.materialise(ids)
                    t1 = time.perf_counter()
                    if r >= warmup:
                        dev[g].append(eng.last_materialise_ms)
                        wall[g].append((t1 - t0) * 1e3)
            for g in LANES:
                print(json.dumps(dict(metric="list_kernel_lanes", workload=name, candidates=select.n_candidates, k=k, n=len(ids), lanes=g,
                                      list_kernel=med(dev[g]), materialise_and_read_wall=med(wall[g]))), flush=True)
            eng.set_materialise_lanes(1)


def batch_rows(name, n_agents, grid, n_obstacles, reps, warmup, k=32):
    """one batch call against the loop of per-agent calls: the kernels (the events around the launches, summed over the loop's
    calls), the calls alone (wall, until the last launch is enqueued, no event read in the timed region) and the calls with the
    per-agent read-back behind them (wall)"""
    from frenetix_motion_planner_amd._lib import check, lib
    inps = [synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=8.0 + 0.1 * a, seed=100 + a, n_pred=30, grid=grid,
                                  n_obstacles=n_obstacles, write_bundle=False, write_costmap=False) for a in range(n_agents)]
    cap = max(i.n_candidates for i in inps) + 64
    with FrenetEngine(max_candidates=cap * n_agents, max_steps=inps[0].N, max_agents=n_agents) as eng:
        res = eng.plan_batch(inps)
        top = eng.topk(k)[1]
        ids = [np.unique(np.concatenate([[res[a]["best_index"]], top[a][top[a] >= 0]]).astype(np.int64)) for a in range(n_agents)]
        ids = [x[x >= 0] for x in ids]
        ids = [x if len(x) else np.arange(k + 1, dtype=np.int64) for x in ids]   # (an agent without a survivor: its first k + 1 candidates)
        agents = list(range(n_agents))
        lists = [ids[a] for a in agents]
        L = lib()

        ag = np.asarray(agents, np.int32)
        n_ids = np.asarray([len(x) for x in lists], np.int64)
        addr = np.asarray([x.ctypes.data for x in lists], np.uint64)

        def loop_calls(timed_kernels):
            """the per-agent calls; with timed_kernels the events of every call are read (a wait per call) and summed"""
            ms = 0.0
            for a, x in zip(agents, lists):
                check(L.fx_materialise_candidates_agent(eng._ctx, a, len(x), x.ctypes.data))
                if timed_kernels:
                    ms += eng.last_materialise_ms
            return ms

        def batch_call(timed_kernels):
            check(L.fx_materialise_candidates_batch(eng._ctx, len(agents), ag.ctypes.data, n_ids.ctypes.data, addr.ctypes.data))
            return eng.last_materialise_ms if timed_kernels else 0.0

        legs = [(form, g) for g in LANES for form in ("loop", "batch")]
        out = {leg: dict(dev=[], call=[], read=[], info=None) for leg in legs}
        for r in range(reps + warmup):
            for form, g in legs:
                eng.set_materialise_lanes(g)
                calls = loop_calls if form == "loop" else batch_call
                # (a) the calls alone, until the last launch is enqueued: no event is read inside the timed region (a per-agent call
                #     waits for the stream at its start, so the loop's figure holds every kernel but its last; the batch's holds none)
                t0 = time.perf_counter()     # (the stream is idle: the leg before ended in a read-back)
                calls(False)
                t1 = time.perf_counter()
                eng.last_materialise_ms      # (waits for the last launch, outside the timed region)
                # (b) the kernels, from the events around the launches
                ms = calls(True)
                out[(form, g)]["info"] = eng.last_materialise_info
                if r >= warmup:
                    out[(form, g)]["dev"].append(ms)
                    out[(form, g)]["call"].append((t1 - t0) * 1e3)
                # (c) the whole of what a planner batch waits for: the calls and every agent's rows read back
                t0 = time.perf_counter()
                if form == "loop":
                    for a, x in zip(agents, lists):
                        eng.materialise(x, agent=a)
                else:
                    eng.materialise_batch(lists, agents=agents)
                t1 = time.perf_counter()
                if r >= warmup:
                    out[(form, g)]["read"].append((t1 - t0) * 1e3)
        for form, g in legs:
            o = out[(form, g)]
            print(json.dumps(dict(metric="materialise_batch", workload=name, agents=len(agents), candidates=inps[0].n_candidates, k=k, form=form,
                                  lanes=g, last_call=o["info"], list_kernels=med(o["dev"]),
                                  calls_wall=med(o["call"]), calls_and_read_wall=med(o["read"]))), flush=True)
        eng.set_materialise_lanes(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-1m", action="store_true")
    ap.add_argument("--trace-workload", action="store_true")
    ap.add_argument("--lanes-batch", action="store_true")
    a = ap.parse_args()
    if a.lanes_batch:
        lanes_rows("config3", WORK["config3"], (32, 64, 800), a.reps, a.warmup)
        if not a.skip_1m:
            lanes_rows("north_star_1m", WORK["north_star_1m"], (64,), a.reps, a.warmup)
        for name, b in BATCHES.items():
            batch_rows(name, b["n_agents"], b["grid"], b["n_obstacles"], a.reps, a.warmup)
        return
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
