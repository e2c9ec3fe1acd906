#!/usr/bin/env python3
"""A finished plan step re-evaluated under H prediction sets in one call (FrenetEngine.hypotheses) against what a
caller does without it, measured in one process on one resident step.  One JSON line per (size, H).

  config3   19 x 51 x 51 (+ d0) = 50 388 candidates, 20 obstacles
  planner   5 x 9 x 13 (+ d0) = 630 candidates, 5 obstacles          (the planner's operating point)
  H         1, 4, 16, 64 hypotheses: the step's own predictions, then every obstacle shifted by a seeded offset of sigma = 0.5 m
            (positions and hulls) and its covariance inflated by a seeded factor in [1, 4]

Per (size, H), after --warmup repetitions, p5 / p50 / p95 of --reps, the legs alternating within a repetition:
  call_wall      host clock around one hypotheses(H) call (tables packed, one copy up, launches, answers back)
  call_device    device time of its launches (events; fx_last_hypotheses_ms)
  steps_wall     host clock around the loop of H update_step calls with those arrays on a second engine -- what a caller does
                 without the pass; the FxStateUpdate structs are built beforehand
The winners of the two legs are compared once per (size, H)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = dict(config3=((19, 51, 51), 20), planner=((5, 9, 13), 5))
N_HYPS = (1, 4, 16, 64)


def stats(xs_ms):
    xs = np.asarray(xs_ms, float) * 1e3
    return dict(p5_us=float(np.percentile(xs, 5)), p50_us=float(np.median(xs)), p95_us=float(np.percentile(xs, 95)), reps=len(xs))


def hypotheses(own, H):
    """H hypothesis arrays: own first, the others shifted and inflated"""
    out = [own]
    for h in range(1, H):
        rng = np.random.default_rng([20251021, h])
        hyp = copy.deepcopy(own)
        shift = rng.normal(0.0, 0.5, size=(own["K"], 1, 2))
        hyp["pos"] = hyp["pos"] + shift
        hyp["hull"][:, :, 0:2] += shift
        hyp["cov_inv"] = hyp["cov_inv"] / rng.uniform(1.0, 4.0, size=(own["K"], 1, 1))
        out.append(hyp)
    return out


def run(size, n_hyps, reps, warmup):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from frenetix_motion_planner_amd.problem import hypothesis_arrays
    grid, n_obst = SIZES[size]
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, grid=grid, n_obstacles=n_obst, lead_gap=25.0)
    mk = lambda: FrenetEngine(max_candidates=inp.n_candidates + 64, max_steps=inp.N, max_obstacles=32, max_pred_steps=64)
    own = hypothesis_arrays(inp.obstacles, inp.obstacles["K"], inp.obstacles["P"])
    with mk() as eng, mk() as eng2:
        eng.plan_step(inp)
        eng2.plan_step(inp)
        split = bool(eng.step_info()["obstacle_kernel"])
        for H in n_hyps:
            hyps = hypotheses(own, H)
            updates = [eng2.make_state_update(obstacles=h) for h in hyps]
            legs = dict(call_wall=[], call_device=[], steps_wall=[])
            for r in range(reps + warmup):
                t0 = time.perf_counter()
                got = eng.hypotheses(hyps)
                t1 = time.perf_counter()
                dev = eng.last_hypotheses_ms
                t2 = time.perf_counter()
                steps = [int(eng2.update_step_raw(u)[0].best_index) for u in updates]
                t3 = time.perf_counter()
                if r == 0:
                    assert np.array_equal(got["winner"], np.array(steps) - inp.shard_begin), (got["winner"][:8], steps[:8])
                if r >= warmup:
                    for k, v in zip(legs, ((t1 - t0) * 1e3, dev, (t3 - t2) * 1e3)):
                        legs[k].append(v)
            info = eng.last_hypotheses_info
            print(json.dumps(dict(metric="hypotheses", size=size, candidates=inp.n_candidates, obstacles=n_obst, n_hyp=H, split_step=split,
                                  distinct_winners=len(set(got["winner"].tolist())), **info, **{k: stats(v) for k, v in legs.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES), action="append")
    ap.add_argument("--n-hyp", type=int, action="append")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for size in a.size or ("config3", "planner"):
        run(size, tuple(a.n_hyp or N_HYPS), a.reps, a.warmup)


if __name__ == "__main__":
    main()
