#!/usr/bin/env python3
"""The re-score of a whole agent batch: one `FrenetEngine.rescore_batch` call against the loop of per-agent `rescore` calls it
replaces, on the same resident step, in one process.  One JSON line per (workload, W).

Workloads:
  a  32 agents of the planner's operating point: 5 x 9 x 13 (+ d0) = 630 candidates, 4 obstacles each      W = 1, 16, 256
  b  BASELINE config 4's shape: 5 agents x the dense 19 x 23 x 23 (+ d0) grid = 10 488 candidates          W = 16
  r  config 3: 19 x 51 x 51 (+ d0) = 50 388 candidates, one agent, W = 16: the per-agent call WITH external rows
     (fx_rescore_agent_rows: a prediction row and a responsibility row) against the plain one (fx_rescore_agent) -- what the table of
     row pointers costs

Per (workload, W), after --warmup repetitions, p5 / p50 / p95 of --reps, the legs alternating within a repetition:
  batch_wall, batch_device     host clock around one rescore_batch call; device time of its launches (fx_last_rescore_ms)
  loop_wall, loop_device       the same around the loop of rescore(agent=a) calls; their device times summed (a second loop)
  (workload r: rows_wall, rows_device against plain_wall, plain_device)
The winners and costs of both legs are compared in every repetition (workload r: the rows are zeros and the responsibility weight is
one, so the winners are the plain call's).

    python tools/bench_rescore_batch.py [--workloads a,b,r] [--reps 20] [--out profiles/rescore_batch/bench_rescore_batch.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_VECS = dict(a=(1, 16, 256), b=(16,), r=(16,))


def workload(name):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    mk = lambda **kw: synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", **kw)
    if name == "a":
        return [mk(v0=8.0 + 0.2 * a, grid=(5, 9, 13), n_obstacles=4) for a in range(32)]
    if name == "b":
        return [mk(v0=8.0 + a, grid=(19, 23, 23), n_obstacles=4) for a in range(5)]
    return [mk(v0=10.0, n_pred=30, grid=(19, 51, 51), n_obstacles=20, lead_gap=25.0)]


def stats(xs_ms):
    xs = np.asarray(xs_ms, float) * 1e3
    return dict(p5_us=float(np.percentile(xs, 5)), p50_us=float(np.median(xs)), p95_us=float(np.percentile(xs, 95)), reps=len(xs))


def weights(inp, W, a, extra=0):
    rng = np.random.default_rng([20251022, W, a])
    base = np.concatenate([inp._cost_w, np.ones(extra)])
    w = base[None, :] * 10.0 ** rng.uniform(-0.5, 0.5, size=(W, len(base)))
    w[0] = base
    return w


def same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g["winner"], w["winner"]) and np.array_equal(g["cost"].view(np.int64), w["cost"].view(np.int64))


def run(name, reps, warmup, out):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inps = workload(name)
    n = len(inps)
    with FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in inps), max_steps=max(i.N for i in inps), max_obstacles=32,
                      max_pred_steps=64, max_agents=n) as eng:
        eng.plan_batch(inps)
        for W in N_VECS[name]:
            if name == "r":
                inp = inps[0]
                zeros = np.zeros(inp.n_candidates)
                k = inp.cost_names.index("prediction")
                plain_w = weights(inp, W, 0)
                rows_w = np.insert(plain_w, k + 1, 1.0, axis=1)            # the responsibility term behind the prediction
                pred = np.ascontiguousarray(eng.costmap()[:, k])           # the step's own prediction row, from outside
                legs = dict(rows_wall=[], rows_device=[], plain_wall=[], plain_device=[])
                for r in range(reps + warmup):
                    t0 = time.perf_counter()
                    got = eng.rescore(rows_w, pred=pred, resp=zeros)
                    t1 = time.perf_counter()
                    d_rows = eng.last_rescore_ms
                    t2 = time.perf_counter()
                    want = eng.rescore(plain_w)
                    t3 = time.perf_counter()
                    d_plain = eng.last_rescore_ms
                    assert np.array_equal(got["winner"], want["winner"])
                    if r >= warmup:
                        for key, v in zip(legs, ((t1 - t0) * 1e3, d_rows, (t3 - t2) * 1e3, d_plain)):
                            legs[key].append(v)
            else:
                ws = [weights(inp, W, a) for a, inp in enumerate(inps)]
                legs = dict(batch_wall=[], batch_device=[], loop_wall=[], loop_device=[])
                for r in range(reps + warmup):
                    t0 = time.perf_counter()
                    got = eng.rescore_batch(ws)
                    t1 = time.perf_counter()
                    d_batch = eng.last_rescore_ms
                    t2 = time.perf_counter()
                    want = [eng.rescore(ws[a], agent=a) for a in range(n)]
                    t3 = time.perf_counter()
                    same(got, want)
                    d_loop = 0.0
                    for a in range(n):       # (the device times in a loop of their own: reading one waits for its events)
                        eng.rescore(ws[a], agent=a)
                        d_loop += eng.last_rescore_ms
                    if r >= warmup:
                        for key, v in zip(legs, ((t1 - t0) * 1e3, d_batch, (t3 - t2) * 1e3, d_loop)):
                            legs[key].append(v)
            line = json.dumps(dict(metric="rescore_batch", workload=name, agents=n, candidates=inps[0].n_candidates, n_vec=W,
                                   **{k: stats(v) for k, v in legs.items()}))
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,r")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    for name in a.workloads.split(","):
        run(name, a.reps, a.warmup, a.out)


if __name__ == "__main__":
    main()
