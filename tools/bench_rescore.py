#!/usr/bin/env python3
"""A finished plan step re-scored under W weight vectors in one call (FrenetEngine.rescore) against what a
caller does without it, measured in one process on one resident step.  One JSON line per (size, W).

  config3   19 x 51 x 51 (+ d0) = 50 388 candidates, 20 obstacles
  planner   5 x 9 x 13 (+ d0) = 630 candidates, 5 obstacles          (the planner's operating point)
  W         1, 16, 256 weight vectors: the default weights, each term scaled by a seeded factor in [10^-0.5, 10^0.5]

Per (size, W), after --warmup repetitions, p5 / p50 / p95 of --reps, the legs alternating within a repetition:
  rescore_wall       host clock around one rescore(W) call (weights up, launches, winners and costs back)
  rescore_device     device time of its launches (events; fx_last_rescore_ms)
  lane_device, vector_device   the same call forced into either regime (fx_rescore_set_regime): where the switch stands
  steps_wall         host clock around the loop of W plan_step calls with those weights on a second engine -- what a caller does
                     today; the PlanInputs are built beforehand
  host_wall          host clock around costmap() + flags read back and the NumPy re-sum and arg-min of the W vectors
The winners of the three paths are compared once per (size, W) (the host's sums are NumPy's: the same operations, see
tests/rescore_planes.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = dict(config3=((19, 51, 51), 20), planner=((5, 9, 13), 5))
N_VECS = (1, 16, 256)


def stats(xs_ms):
    xs = np.asarray(xs_ms, float) * 1e3
    return dict(p5_us=float(np.percentile(xs, 5)), p50_us=float(np.median(xs)), p95_us=float(np.percentile(xs, 95)), reps=len(xs))


def run(size, n_vecs, reps, warmup):
    from frenetix_motion_planner_amd import _abi, synthetic
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
    grid, n_obst = SIZES[size]
    kw = dict(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, grid=grid, n_obstacles=n_obst, lead_gap=25.0)
    inp = synthetic.make_inputs(**kw)
    names = inp.cost_names
    n_pred = names.index("prediction")
    mk = lambda: FrenetEngine(max_candidates=inp.n_candidates + 64, max_steps=inp.N, max_obstacles=32, max_pred_steps=64)
    sel = _abi.FX_FLAG_SELECTABLE
    bad = _abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY
    with mk() as eng, mk() as eng2:
        eng.plan_step(inp)
        deferred = bool(eng.step_info()["obstacle_kernel"])
        for W in n_vecs:
            rng = np.random.default_rng([20251021, W])
            w = inp._cost_w[None, :] * 10.0 ** rng.uniform(-0.5, 0.5, size=(W, len(names)))
            w[0] = inp._cost_w
            others = [synthetic.make_inputs(cost_weights=dict(zip(names, row)), **kw) for row in w]

            def host():
                raw, (_, flags) = eng.costmap(), eng.costs()
                ok = ((flags & sel) != 0) & ((flags & bad) == 0) & ((flags & _abi.FX_FLAG_COSTED) != 0)
                win = np.empty(W, np.int64)
                for k in range(W):
                    s, tail = np.full(len(raw), -0.0), np.zeros(len(raw))
                    for m in range(len(names)):
                        t = w[k, m] * raw[:, m]
                        if deferred and m > n_pred:
                            tail = tail + t
                        else:
                            s = s + t
                    total = 0.0 + (s + tail if deferred and n_pred + 1 < len(names) else s)
                    el = np.nonzero(ok & ~np.isnan(total))[0]
                    win[k] = int(el[np.argmin(total[el])]) if len(el) else -1      # (argmin: the first of equals, the lowest index)
                return win

            def forced(regime):
                lib().fx_rescore_set_regime(regime)
                try:
                    eng.rescore(w)
                    return eng.last_rescore_ms
                finally:
                    lib().fx_rescore_set_regime(0)

            legs = dict(rescore_wall=[], rescore_device=[], lane_device=[], vector_device=[], steps_wall=[], host_wall=[])
            for r in range(reps + warmup):
                t0 = time.perf_counter()
                got = eng.rescore(w)
                t1 = time.perf_counter()
                dev = eng.last_rescore_ms
                d_lane, d_vec = forced(1), forced(2)
                t2 = time.perf_counter()
                steps = [eng2.plan_step(o)["best_index"] for o in others]
                t3 = time.perf_counter()
                want = host()
                t4 = time.perf_counter()
                if r == 0:
                    assert np.array_equal(got["winner"], steps) and np.array_equal(got["winner"], want), (got["winner"][:8], steps[:8], want[:8])
                if r >= warmup:
                    for k, v in zip(legs, ((t1 - t0) * 1e3, dev, d_lane, d_vec, (t3 - t2) * 1e3, (t4 - t3) * 1e3)):
                        legs[k].append(v)
            print(json.dumps(dict(metric="rescore", size=size, candidates=inp.n_candidates, n_vec=W, regime=int(lib().fx_rescore_regime(inp.n_candidates, W)),
                                  deferred=deferred, distinct_winners=len(set(got["winner"].tolist())), **{k: stats(v) for k, v in legs.items()})),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", choices=sorted(SIZES), action="append")
    ap.add_argument("--n-vec", type=int, action="append")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    for size in a.size or ("config3", "planner"):
        run(size, tuple(a.n_vec or N_VECS), a.reps, a.warmup)


if __name__ == "__main__":
    main()
