"""The collision-probability pass of a whole agent batch: one `FrenetEngine.prediction_probability_batch` call against the loop of
`prediction_probability(agent=a)` calls it replaces, on the same resident step, obstacles and process.

Workloads:
  a  32 agents of the reference's operating point: 630 candidates x 31 samples, 5 obstacles each
  b  BASELINE config 4's shape: 5 agents x the dense 19 x 23 x 23 (+ d0) grid = 10 488 candidates, 5 obstacles each
  c  4 agents of BASELINE config 5's shape: 103 428 candidates x 51 samples, 20 obstacles each (bound by the BVN evaluations)
Per workload the two variants alternate --reps times after a warm-up; wall time around the call(s) and device time
(`last_predprob_ms`, summed over the loop) are reported as median and p5 / p25 / p75 / p95, one JSON line per workload, and the
decision rule of AgentBatchHip(batched_passes=None) is evaluated over a and b: on only if the batched call's wall p95 lies below
the loop's wall p5 at both.

    python tools/bench_predprob_batch.py [--workloads a,b,c] [--reps 20] [--out profiles/predprob_batch/bench.jsonl]
    python tools/bench_predprob_batch.py --workloads a --batched-only 10      # for a kernel trace: ten batched calls, nothing else
    python tools/bench_predprob_batch.py --workloads a,b --chunk-steps 4      # both variants with that many steps per chunk
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
from tests.test_risk_gpu import _predictions  # noqa: E402

EGO_L, EGO_W = 4.508, 1.61


def workload(name):
    """(inputs of the agents, obstacles per agent)"""
    if name == "a":
        return [synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=8.0 + 0.2 * a, grid=(6, 15, 6), n_obstacles=4)
                for a in range(32)], 5
    if name == "b":
        return [synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=8.0 + a, grid=(19, 23, 23), n_obstacles=4)
                for a in range(5)], 5
    return synthetic.stress_agents(4, hull_builder=build_obstacle_hulls, write_bundle=True), 20


def pcts(v):
    p = np.percentile(np.asarray(v, np.float64), [50, 5, 25, 75, 95])
    return dict(median=float(p[0]), p5=float(p[1]), p25=float(p[2]), p75=float(p[3]), p95=float(p[4]))


def one(name, reps, warmup, batched_only):
    inps, K = workload(name)
    n = len(inps)
    with FrenetEngine(max_candidates=sum(i.n_candidates for i in inps), max_steps=max(i.n_samples for i in inps) - 1, max_ref_knots=4096,
                      max_obstacles=32, max_pred_steps=max(64, max(i.n_samples for i in inps) + 1), device=0, max_agents=n) as eng:
        eng.plan_batch(inps)
        for a in range(n):
            _, flags = eng.costs(a)
            planes = {p: eng.plane(p, a).T.copy() for p in ("x", "y", "theta", "v")}
            preds, typ = _predictions(planes, flags, np.random.default_rng(100 + a), n_obs=K)
            eng.set_risk_obstacles(risk.obstacle_tables(preds, typ), a)
            del planes

        def loop():
            t0, dev, out = time.perf_counter(), 0.0, []
            for a in range(n):
                out.append(eng.prediction_probability(EGO_L, EGO_W, agent=a))
                dev += eng.last_predprob_ms
            return (time.perf_counter() - t0) * 1e3, dev, out

        def batched():
            t0 = time.perf_counter()
            out = eng.prediction_probability_batch(EGO_L, EGO_W)
            return (time.perf_counter() - t0) * 1e3, eng.last_predprob_ms, out

        if batched_only:
            for _ in range(batched_only):
                batched()
            return dict(metric=f"prediction_probability_batch only, workload {name}", calls=batched_only)
        for _ in range(warmup):
            _, _, want = loop()
            _, _, got = batched()
        same = all(np.array_equal(g[k], w[k], equal_nan=True) for g, w in zip(got, want) for k in ("prob", "total")) and \
            all(g["best_index"] == w["best_index"] for g, w in zip(got, want))
        lw, ld, bw, bd = [], [], [], []
        for _ in range(reps):
            w, d, _ = loop()
            lw.append(w), ld.append(d)
            w, d, _ = batched()
            bw.append(w), bd.append(d)
    return dict(metric=f"prediction_probability: per-agent loop against one batched call, workload {name}", agents=n,
                candidates=sorted({i.n_candidates for i in inps}),
                steps=inps[0].n_samples, obstacles=K, reps=reps, same_bits=bool(same),
                loop_wall_ms=pcts(lw), batch_wall_ms=pcts(bw), loop_device_ms=pcts(ld), batch_device_ms=pcts(bd),
                wall_speedup_median=float(np.median(lw) / np.median(bw)), device_speedup_median=float(np.median(ld) / np.median(bd)),
                batch_p95_below_loop_p5=bool(np.percentile(bw, 95) < np.percentile(lw, 5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,c")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batched-only", type=int, default=0, help="only that many batched calls per workload (for a kernel trace)")
    ap.add_argument("--chunk-steps", type=int, default=0, help="force the steps per chunk of both variants (0: the rule of fx_item_chunk_steps)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    lines = []
    from frenetix_motion_planner_amd._lib import lib
    lib().fx_predprob_set_chunk_steps(a.chunk_steps)
    for name in a.workloads.split(","):
        lines.append(dict(one(name, a.reps, a.warmup, a.batched_only), chunk_steps_forced=a.chunk_steps))
    rule = [r["batch_p95_below_loop_p5"] for r in lines if r["metric"].endswith(("workload a", "workload b")) and "batch_p95_below_loop_p5" in r]
    if len(rule) == 2:
        lines.append(dict(metric="batched_passes default by the decision rule (wall p95 of the batched call below wall p5 of the loop at a and b)",
                          default_on=bool(all(rule))))
    for r in lines:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
