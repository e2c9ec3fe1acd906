"""The risk walk in the item decomposition (fx_risk_items_kernel.h) against the walk: `FrenetEngine.risk`,
`risk_detail` and `responsibility_cost` with set_risk_decomposition "items" and "walk" alternating on the same step, obstacles and
process.  The yardstick is the walk, never the items against themselves; the responsibility pass always runs its detail pass as
items, so its yardstick is risk_costs() with the walk -- the same columns and the same cost kernel, without the re-sum.

Two sizes: the planner size (grid (8, 16, 16), 8 obstacles) and BASELINE config 3 (50 388 candidates, the 20 obstacles of
tools/bench_risk.py).  Prints one JSON line per size and call: the median, minimum and maximum of --reps device-event times (all
kernels of the call), the (candidate, obstacle, step) triples that pass the 5 m gate among the evaluated candidates, the BVN
evaluations behind them and the time per 1 000 of them, steps per chunk and items of the pass, its device bytes.  The time limit
(--limit seconds of wall time per size) is looked at between calls: a size that runs over is given up, and said so, but a call
that never returns is not ended by it -- everything runs in this one process, so run the tool under `timeout` for that.

    timeout -k 10 600 python tools/bench_risk_items.py [--reps 20] [--limit 120] [--out profiles/risk_items/bench.jsonl]
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
from frenetix_motion_planner_amd._lib import lib  # noqa: E402
from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls  # noqa: E402
from tests.test_risk_gpu import _predictions, HARM, BASE, EGO  # noqa: E402
from tools.bench_predprob import gated_triples  # noqa: E402

SIZES = {"planner size": dict(grid=(8, 16, 16), n_obstacles=4, n_obs=8, seed=7),
         "config 3": dict(grid=(19, 51, 51), n_obstacles=20, n_obs=20, seed=3)}


def one(name, cfg, reps, limit):
    t_end = time.monotonic() + limit
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=cfg["grid"], n_obstacles=cfg["n_obstacles"])
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        _, flags = eng.costs()
        planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(cfg["seed"]), n_obs=cfg["n_obs"])
        eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
        params = risk.risk_params(dict(BASE), HARM, **EGO)
        resp = risk.action_space_responsibility(preds, np.array([planes["x"][0, 0], planes["y"][0, 0]]), float(planes["theta"][0, 0]))
        cost = lambda: risk.risk_cost_params([0, 0, 0, 0, 1], responsibility=resp)
        calls = {"risk": (lambda: eng.risk(params), lambda: eng.risk(params)),
                 "risk_detail": (lambda: eng.risk_detail(params), lambda: eng.risk_detail(params)),
                 "responsibility_cost against risk_costs": (lambda: eng.responsibility_cost(params, cost(), 0.5), lambda: eng.risk_costs(params, cost()))}
        before = eng.device_bytes
        S, K = inp.n_samples, len(preds)
        sel = np.nonzero((flags & 0xB) == 0xB)[0]
        gated = gated_triples(planes, sel, preds)
        cs = int(lib().fx_risk_items_chunk_steps(inp.n_candidates, S, K))
        for call, (items, walk) in calls.items():
            ms = {"items": [], "walk": []}
            for rep in range(reps + 1):   # (the first round: allocation, first launch)
                for mode, fn in (("items", items), ("walk", walk)):
                    if time.monotonic() > t_end:
                        yield dict(metric=f"{call}, {name}", gave_up=f"more than {limit} s of wall time")
                        return
                    eng.set_risk_decomposition(mode)
                    fn()
                    if rep:
                        ms[mode].append(eng.last_risk_ms)
            med = {m: float(np.median(v)) for m, v in ms.items()}
            yield dict(metric=f"{call}, items against walk, {name}", candidates=inp.n_candidates, evaluated=int(len(sel)), obstacles=K, steps=S,
                       reps=reps, items_ms_median=med["items"], items_ms_min=float(np.min(ms["items"])), items_ms_max=float(np.max(ms["items"])),
                       walk_ms_median=med["walk"], walk_ms_min=float(np.min(ms["walk"])), walk_ms_max=float(np.max(ms["walk"])),
                       speedup=med["walk"] / med["items"], gated_triples=gated, bvn_evaluations=36 * gated,
                       items_us_per_1000_bvn=med["items"] * 1e3 / max(36 * gated / 1000.0, 1e-300),
                       walk_us_per_1000_bvn=med["walk"] * 1e3 / max(36 * gated / 1000.0, 1e-300), steps_per_chunk=cs,
                       items=int(((inp.n_candidates + 63) // 64) * K * ((S - 1 + cs - 1) // cs)), risk_block_bytes=int(eng.device_bytes - before))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=float, default=120.0, help="wall-time limit per size, seconds")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for name, cfg in SIZES.items():
        for rec in one(name, cfg, a.reps, a.limit):
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
