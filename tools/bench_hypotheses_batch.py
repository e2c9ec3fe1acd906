#!/usr/bin/env python3
"""The hypotheses pass of a whole agent batch: one `FrenetEngine.hypotheses_batch` call against the loop of per-agent `hypotheses`
calls it replaces, on the same resident step, in one process.  One JSON line per (workload, H).

Workloads:
  a  32 agents of the planner's operating point: 5 x 9 x 13 (+ d0) = 630 candidates, 5 obstacles each      H = 1, 4, 16
  b  BASELINE config 4's shape: 5 agents x the dense 19 x 23 x 23 (+ d0) grid = 10 488 candidates          H = 4
  c  4 agents of BASELINE config 5's shape: 39 x 51 x 51 (+ d0) = 103 428 candidates x 51 samples, 20 obstacles each    H = 4
  H  hypotheses per agent: the step's own predictions, then every obstacle shifted by a seeded offset of sigma = 0.5 m (positions
     and hulls) and its covariance inflated by a seeded factor in [1, 4] (tools/bench_hypotheses.py's sets)

Per (workload, H), after --warmup repetitions, p5 / p50 / p95 of --reps, the legs alternating within a repetition:
  batch_wall, batch_device     host clock around one hypotheses_batch call; device time of its launches (fx_last_hypotheses_ms)
  loop_wall, loop_device       the same around the loop of hypotheses(agent=a) calls -- what a caller does without the batch call;
                               their device times summed (a second loop: reading one waits for its events)
The winners, costs and collision counts of both legs are compared in every repetition.

    python tools/bench_hypotheses_batch.py [--workloads a,b,c] [--reps 20] [--out profiles/hypotheses_batch/bench_hypotheses_batch.jsonl]"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_HYPS = dict(a=(1, 4, 16), b=(4,), c=(4,))


def workload(name):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    mk = lambda **kw: synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", lead_gap=25.0, **kw)
    if name == "a":
        return [mk(v0=8.0 + 0.2 * a, n_pred=30, grid=(5, 9, 13), n_obstacles=5) for a in range(32)]
    if name == "b":
        return [mk(v0=8.0 + a, n_pred=30, grid=(19, 23, 23), n_obstacles=4) for a in range(5)]
    return [mk(v0=9.0 + a, horizon=5.0, n_pred=50, grid=(39, 51, 51), n_obstacles=20) for a in range(4)]


def stats(xs_ms):
    xs = np.asarray(xs_ms, float) * 1e3
    return dict(p5_us=float(np.percentile(xs, 5)), p50_us=float(np.median(xs)), p95_us=float(np.percentile(xs, 95)), reps=len(xs))


def hypotheses(own, H, a):
    """H hypothesis arrays of agent a: own first, the others shifted and inflated"""
    out = [own]
    for h in range(1, H):
        rng = np.random.default_rng([20251021, h, a])
        hyp = copy.deepcopy(own)
        shift = rng.normal(0.0, 0.5, size=(own["K"], 1, 2))
        hyp["pos"] = hyp["pos"] + shift
        hyp["hull"][:, :, 0:2] += shift
        hyp["cov_inv"] = hyp["cov_inv"] / rng.uniform(1.0, 4.0, size=(own["K"], 1, 1))
        out.append(hyp)
    return out


def same(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g["winner"], w["winner"]) and np.array_equal(g["cost"].view(np.int64), w["cost"].view(np.int64))
        assert np.array_equal(g["n_collisions"], w["n_collisions"])


def run(name, reps, warmup, out):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from frenetix_motion_planner_amd.problem import hypothesis_arrays
    inps = workload(name)
    n = len(inps)
    with FrenetEngine(max_candidates=sum(i.n_candidates + 64 for i in inps), max_steps=max(i.N for i in inps), max_obstacles=32,
                      max_pred_steps=64, max_agents=n) as eng:
        results = eng.plan_batch(inps)
        split = bool(eng.step_info()["obstacle_kernel"])
        own = [hypothesis_arrays(i.obstacles, i.obstacles["K"], i.obstacles["P"]) for i in inps]
        for H in N_HYPS[name]:
            sets = [hypotheses(own[a], H, a) for a in range(n)]
            legs = dict(batch_wall=[], batch_device=[], loop_wall=[], loop_device=[])
            for r in range(reps + warmup):
                t0 = time.perf_counter()
                got = eng.hypotheses_batch(sets)
                t1 = time.perf_counter()
                d_batch = eng.last_hypotheses_ms
                info = eng.last_hypotheses_info
                t2 = time.perf_counter()
                want = [eng.hypotheses(sets[a], agent=a) for a in range(n)]
                t3 = time.perf_counter()
                same(got, want)
                d_loop = 0.0
                for a in range(n):       # (the device times in a loop of their own: reading one waits for its events)
                    eng.hypotheses(sets[a], agent=a)
                    d_loop += eng.last_hypotheses_ms
                if r >= warmup:
                    for key, v in zip(legs, ((t1 - t0) * 1e3, d_batch, (t3 - t2) * 1e3, d_loop)):
                        legs[key].append(v)
            s = {k: stats(v) for k, v in legs.items()}
            line = json.dumps(dict(metric="hypotheses_batch", workload=name, agents=n, candidates=inps[0].n_candidates,
                                   samples=inps[0].n_samples, obstacles=int(inps[0].obstacles["K"]), n_hyp=H, split_step=split,
                                   own_winner_is_the_steps=bool(all(abs(int(g["winner"][0]) - (r_["best_index"] - i.shard_begin)) == 0
                                                                    for g, r_, i in zip(got, results, inps))),
                                   distinct_winners=len({int(w) for g in got for w in g["winner"]}), **info,
                                   batch_wins=bool(s["batch_wall"]["p95_us"] < s["loop_wall"]["p5_us"]), **s))
            print(line, flush=True)
            if out:
                with open(out, "a") as f:
                    f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,c")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.workloads.split(","):
        run(name, a.reps, a.warmup, a.out)


if __name__ == "__main__":
    main()
