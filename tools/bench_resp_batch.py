"""The responsibility pass of a whole agent batch: one `FrenetEngine.responsibility_cost_batch` call against the loop of
`responsibility_cost(agent=a)` calls it replaces, on the same resident step, obstacles and process.

Workloads (those of tools/bench_predprob_batch.py):
  a  32 agents of the reference's operating point: 630 candidates x 31 samples, 5 obstacles each
  b  BASELINE config 4's shape: 5 agents x the dense 19 x 23 x 23 (+ d0) grid = 10 488 candidates, 5 obstacles each
  c  4 agents of BASELINE config 5's shape: 103 428 candidates x 51 samples, 20 obstacles each
The obstacles walk along the agents' own candidates (tests.test_risk_gpu._predictions), so most items pass the 5 m gate: far heavier
than a planner's usual scene.  The agents alternate between action-space and reach-set mode.  Per workload the two variants
alternate --reps times after a warm-up; wall time around the call(s) and device time (`last_risk_ms`, summed over the loop) are
reported as median and p5 / p25 / p75 / p95, one JSON line per workload, and the decision rule of
AgentBatchHip(batched_responsibility=None) is evaluated over a and b: on only if the batched call's wall p95 lies below the loop's
wall p5 at both.

    python tools/bench_resp_batch.py [--workloads a,b,c] [--reps 20] [--out profiles/resp_batch/bench.jsonl]
    python tools/bench_resp_batch.py --workloads a --batched-only 10      # for a kernel trace: ten batched calls, nothing else
    python tools/bench_resp_batch.py --workloads a,b --chunk-steps 4      # both variants with that many steps per chunk
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
from tests.test_risk_costs_gpu import _reach_sets  # noqa: E402
from tests.test_risk_gpu import BASE, EGO, HARM, _predictions  # noqa: E402
from tools.bench_predprob_batch import pcts, workload  # noqa: E402

W_RESP = 0.5
KEYS = ("resp", "total", "ego_risk", "obst_risk")


def one(name, reps, warmup, batched_only):
    inps, K = workload(name)
    n = len(inps)
    params = risk.risk_params(BASE, HARM, **EGO)
    with FrenetEngine(max_candidates=sum(i.n_candidates for i in inps), max_steps=max(i.n_samples for i in inps) - 1, max_ref_knots=4096,
                      max_obstacles=32, max_pred_steps=max(64, max(i.n_samples for i in inps) + 1), device=0, max_agents=n) as eng:
        eng.plan_batch(inps)
        costs = []
        for a in range(n):
            _, flags = eng.costs(a)
            planes = {p: eng.plane(p, a).T.copy() for p in ("x", "y", "theta", "v")}
            preds, typ = _predictions(planes, flags, np.random.default_rng(100 + a), n_obs=K)
            keys = list(preds)
            ok = np.nonzero((flags & 0xB) == 0xB)[0]
            eng.set_risk_obstacles(risk.obstacle_tables(preds, typ), a)
            if a % 2:
                eng.set_reach_sets(risk.reach_set_tables(_reach_sets(planes, keys, ok[::3], inps[a].dt), keys, inps[a].dt, inps[a].n_samples), a)
                resp = "reach_set"
            else:
                resp = risk.action_space_responsibility(preds, np.array([planes["x"][ok[0], 0], planes["y"][ok[0], 0]]),
                                                        float(planes["theta"][ok[0], 0]) + 0.5)
            costs.append(risk.risk_cost_params([0, 0, 0, 0, 1], responsibility=resp))
            del planes

        def loop():
            t0, dev, out = time.perf_counter(), 0.0, []
            for a in range(n):
                out.append(eng.responsibility_cost(params, costs[a], W_RESP, agent=a))
                dev += eng.last_risk_ms
            return (time.perf_counter() - t0) * 1e3, dev, out

        def batched():
            t0 = time.perf_counter()
            out = eng.responsibility_cost_batch([params] * n, costs, [W_RESP] * n)
            return (time.perf_counter() - t0) * 1e3, eng.last_risk_ms, out

        if batched_only:
            for _ in range(batched_only):
                batched()
            return dict(metric=f"responsibility_cost_batch only, workload {name}", calls=batched_only)
        for _ in range(warmup):
            _, _, want = loop()
            _, _, got = batched()
        same = all(np.array_equal(g[k], w[k], equal_nan=True) for g, w in zip(got, want) for k in KEYS) and \
            all(g["best_index"] == w["best_index"] for g, w in zip(got, want))
        assert same, "the batched call and the per-agent loop differ"
        lw, ld, bw, bd = [], [], [], []
        for _ in range(reps):
            w, d, _ = loop()
            lw.append(w), ld.append(d)
            w, d, _ = batched()
            bw.append(w), bd.append(d)
    return dict(metric=f"responsibility_cost: per-agent loop against one batched call, workload {name}", agents=n,
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
    lib().fx_risk_items_set_chunk_steps(a.chunk_steps)
    for name in a.workloads.split(","):
        lines.append(dict(one(name, a.reps, a.warmup, a.batched_only), chunk_steps_forced=a.chunk_steps))
    rule = [r["batch_p95_below_loop_p5"] for r in lines if r["metric"].endswith(("workload a", "workload b")) and "batch_p95_below_loop_p5" in r]
    if len(rule) == 2:
        lines.append(dict(metric="batched_responsibility default by the decision rule (wall p95 of the batched call below wall p5 of the "
                                 "loop at a and b)", default_on=bool(all(rule))))
    for r in lines:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
