"""Risk detail and risk costs of a whole agent batch: one `FrenetEngine.risk_costs_batch` call against the loop of
`risk_costs(agent=a)` calls it replaces, on the same resident step, obstacles and process.

Workloads (the shapes of tools/bench_risk_batch.py, with `risk_costs` in place of `risk`):
  a  32 agents of the reference's operating point: 630 candidates x 31 samples, 5 obstacles each, ONE listed candidate per agent
  b  the same agents without lists
  c  BASELINE config 4's shape: 5 agents x the dense 19 x 23 x 23 (+ d0) grid = 10 488 candidates, 5 obstacles each, without lists
  d  4 agents of BASELINE config 5's shape: 103 428 candidates x 51 samples, 20 obstacles each, without lists
  m  the "min_risk_cost" form: the agents of a, each with the list of every VALID & FEASIBLE & RETURNED candidate
Every agent has cost parameters with all five weights non-zero and the action-space responsibility vector of its own obstacles.
The obstacles walk along the agents' own candidates (tests.test_risk_gpu._predictions), so most items pass the 5 m gate: far heavier
than a planner's usual scene.  Per workload the two variants alternate --reps times after a warm-up; wall time around the call(s)
and device time (`last_risk_ms`, summed over the loop) are reported as median and p5 / p25 / p75 / p95, one JSON line per workload,
and the decision rule of a later AgentBatchHip(batched_risk_costs=None) default is evaluated over a and c: on only if the batched
call's wall p95 lies below the loop's wall p5 at both.

    python tools/bench_risk_costs_batch.py [--workloads a,b,c,d,m] [--reps 20] [--out profiles/risk_costs_batch/bench.jsonl]
    python tools/bench_risk_costs_batch.py --workloads m --batched-only 10      # for a kernel trace: ten batched calls, nothing else
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frenetix_motion_planner_amd import risk  # noqa: E402
from frenetix_motion_planner_amd.engine import FrenetEngine  # noqa: E402
from tests.test_risk_gpu import BASE, EGO, HARM, _predictions  # noqa: E402
from tools.bench_predprob_batch import pcts, workload  # noqa: E402

SHAPE = dict(a=("a", "one"), b=("a", None), c=("b", None), d=("c", None), m=("a", "feasible"))   # (shape of tools/bench_predprob_batch.py, list)
WEIGHTS = [1.0, 0.5, 2.0, 0.25, 1.5]


def _same(got, want):
    return got.keys() == want.keys() and all(
        np.array_equal(np.ascontiguousarray(g).view(np.int64), np.ascontiguousarray(want[k]).view(np.int64)) if isinstance(g, np.ndarray)
        else g == want[k] for k, g in got.items())


def one(name, reps, warmup, batched_only):
    shape, listed = SHAPE[name]
    inps, K = workload(shape)
    n = len(inps)
    params = risk.risk_params(BASE, HARM, **EGO)
    with FrenetEngine(max_candidates=sum(i.n_candidates for i in inps), max_steps=max(i.n_samples for i in inps) - 1, max_ref_knots=4096,
                      max_obstacles=32, max_pred_steps=max(64, max(i.n_samples for i in inps) + 1), device=0, max_agents=n) as eng:
        res = eng.plan_batch(inps)
        ids, costs = [], []
        for a in range(n):
            _, flags = eng.costs(a)
            planes = {p: eng.plane(p, a).T.copy() for p in ("x", "y", "theta", "v")}
            preds, typ = _predictions(planes, flags, np.random.default_rng(100 + a), n_obs=K)
            eng.set_risk_obstacles(risk.obstacle_tables(preds, typ), a)
            ok = np.nonzero((flags & 0xB) == 0xB)[0]
            win = int(res[a]["best_index"])
            ids.append(np.array([win if win >= 0 else int(ok[0])], np.int64) if listed == "one" else (ok if listed else None))
            x0 = np.array([planes["x"][ok[0], 0], planes["y"][ok[0], 0]])
            vec = risk.action_space_responsibility(preds, x0, float(planes["theta"][ok[0], 0]) + 0.5)
            costs.append(risk.risk_cost_params(WEIGHTS, responsibility=vec))
            del planes

        def loop():
            t0, dev, out = time.perf_counter(), 0.0, []
            for a in range(n):
                out.append(eng.risk_costs(params, costs[a], ids[a], agent=a))
                dev += eng.last_risk_ms
            return (time.perf_counter() - t0) * 1e3, dev, out

        def batched():
            t0 = time.perf_counter()
            out = eng.risk_costs_batch(params, costs, ids if listed else None)
            return (time.perf_counter() - t0) * 1e3, eng.last_risk_ms, out

        if batched_only:
            for _ in range(batched_only):
                batched()
            return dict(metric=f"risk_costs_batch only, workload {name}", calls=batched_only)
        for _ in range(warmup):
            _, _, want = loop()
            _, _, got = batched()
        same = all(_same(g, w) for g, w in zip(got, want))
        assert same, "the batched call and the per-agent loop differ"
        rounds = eng.last_risk_costs_batch_rounds
        lw, ld, bw, bd = [], [], [], []
        for _ in range(reps):
            w, d, _ = loop()
            lw.append(w), ld.append(d)
            w, d, _ = batched()
            bw.append(w), bd.append(d)
    return dict(metric=f"risk_costs: per-agent loop against one batched call, workload {name}", agents=n,
                candidates=sorted({i.n_candidates for i in inps}),
                listed=None if not listed else (1 if listed == "one" else [int(min(len(x) for x in ids)), int(max(len(x) for x in ids))]),
                steps=inps[0].n_samples, obstacles=K, reps=reps, rounds=rounds, same_bits=bool(same),
                loop_wall_ms=pcts(lw), batch_wall_ms=pcts(bw), loop_device_ms=pcts(ld), batch_device_ms=pcts(bd),
                wall_speedup_median=float(np.median(lw) / np.median(bw)), device_speedup_median=float(np.median(ld) / np.median(bd)),
                batch_p95_below_loop_p5=bool(np.percentile(bw, 95) < np.percentile(lw, 5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="a,b,c,d,m")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batched-only", type=int, default=0, help="only that many batched calls per workload (for a kernel trace)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    lines = []
    for name in a.workloads.split(","):
        lines.append(one(name, a.reps, a.warmup, a.batched_only))
    rule = [r["batch_p95_below_loop_p5"] for r in lines if r["metric"].endswith(("workload a", "workload c")) and "batch_p95_below_loop_p5" in r]
    if len(rule) == 2:
        lines.append(dict(metric="a later batched_risk_costs default by the decision rule (wall p95 of the batched call below wall p5 of "
                                 "the loop at a and c)", rule_met=bool(all(rule))))
    for r in lines:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
