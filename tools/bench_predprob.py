"""Collision probability as the prediction cost (fx_predprob_kernel.h) against the risk pass that walks the
same probabilities: `FrenetEngine.prediction_probability` and `FrenetEngine.risk` on the same step, obstacles and process.

Two sizes: BASELINE config 3 (50 388 candidates, the 20 obstacles of tools/bench_risk.py) and the planner size (grid
(8, 16, 16), 8 obstacles).  Prints one JSON line per size: the median, minimum and maximum of --reps device-event times of
each call (all its kernels), the (candidate, obstacle, step) triples that pass the 5 m gate among the costed candidates, the
BVN evaluations behind them and the time per 1 000 of them, steps per chunk and items of the pass, its device bytes.
The yardstick, risk(), evaluates the same probabilities plus the harm, one lane per candidate over all records.

    python tools/bench_predprob.py [--reps 20] [--out profiles/predprob/bench_predprob.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frenetix_motion_planner_amd import synthetic, risk  # noqa: E402
from frenetix_motion_planner_amd._lib import lib  # noqa: E402
from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls  # noqa: E402
from tests.test_risk_gpu import _predictions, HARM, BASE, EGO  # noqa: E402

SIZES = {"config 3": dict(grid=(19, 51, 51), n_obstacles=20, n_obs=20, seed=3),
         "planner size": dict(grid=(8, 16, 16), n_obstacles=4, n_obs=8, seed=7)}


def gated_triples(planes, ids, preds):
    S = planes["x"].shape[1]
    x, y = planes["x"][ids], planes["y"][ids]
    gated = 0
    for p in preds.values():
        pos, yaw, ln = p["pos_list"], p["orientation_list"], p["shape"]["length"]
        for i in range(1, min(S, len(pos))):
            dev = np.array([np.cos(yaw[i]), np.sin(yaw[i])]) * ln / 2
            d = np.min([np.hypot(m[0] - x[:, i], m[1] - y[:, i]) for m in (pos[i - 1], pos[i - 1] + dev, pos[i - 1] - dev)], axis=0)
            gated += int(np.count_nonzero(~(d > 5.0)))
    return gated


def one(name, cfg, reps):
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=cfg["grid"], n_obstacles=cfg["n_obstacles"])
    with FrenetEngine(max_candidates=inp.n_candidates, device=0) as eng:
        eng.plan_step(inp)
        _, flags = eng.costs()
        planes = {n: eng.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
        preds, typ = _predictions(planes, flags, np.random.default_rng(cfg["seed"]), n_obs=cfg["n_obs"])
        eng.set_risk_obstacles(risk.obstacle_tables(preds, typ))
        params = risk.risk_params(dict(BASE), HARM, **EGO)
        before = eng.device_bytes
        eng.risk(params)                                                   # allocation, first launch
        eng.prediction_probability(EGO["ego_length"], EGO["ego_width"])
        pp_ms, risk_ms = [], []
        for _ in range(reps):
            eng.prediction_probability(EGO["ego_length"], EGO["ego_width"])
            pp_ms.append(eng.last_predprob_ms)
            eng.risk(params)
            risk_ms.append(eng.last_risk_ms)
        dev_bytes = eng.device_bytes - before
    S, K = inp.n_samples, len(preds)
    costed = np.nonzero(flags & 0x10)[0]
    gated = gated_triples(planes, costed, preds)
    cs = int(lib().fx_predprob_chunk_steps(inp.n_candidates, S, K))
    med = float(np.median(pp_ms))
    return dict(metric=f"prediction_probability against risk, {name}", candidates=inp.n_candidates, costed=int(len(costed)), obstacles=K, steps=S,
                reps=reps, predprob_ms_median=med, predprob_ms_min=float(np.min(pp_ms)), predprob_ms_max=float(np.max(pp_ms)),
                risk_ms_median=float(np.median(risk_ms)), risk_ms_min=float(np.min(risk_ms)), risk_ms_max=float(np.max(risk_ms)),
                speedup=float(np.median(risk_ms)) / med, gated_triples=gated, bvn_evaluations=36 * gated,
                us_per_1000_bvn=med * 1e3 / max(36 * gated / 1000.0, 1e-300), steps_per_chunk=cs,
                items=int(((inp.n_candidates + 63) // 64) * K * ((S - 1 + cs - 1) // cs)), risk_block_bytes=int(dev_bytes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    a = ap.parse_args()
    for name, cfg in SIZES.items():
        line = json.dumps(one(name, cfg, a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
