#!/usr/bin/env python3
"""Batched candidate read-back (fx_read_candidates_agent) against the loop of single read-backs it
replaces, and what keeping samples costs a handler.  One JSON line per measurement; host clock around calls that end in a
stream synchronise, warm-up first, median / p5 / p95 over --reps repetitions.

  read        engine.candidates(ids) vs [engine.candidate(i) for i in ids] in the same process, alternating, on the 800-row
              matrix step of the frenetix route (n = 6, 64, 800) and on golden arc_hv_l4_horizon5_prod_obs8 (n = 800, 22 440;
              the single-read loop of 22 440 -- 1.2 s each -- runs --reps-big times)
  reset       TrajectoryHandler.reset_Trajectories() with 0, 6 and 800 live samples of the 800-row step
  bytes       n x record bytes from the shapes -- over the gather kernel's time this is its achieved bytes/s; the kernel's
              time comes from a trace run of its own:
                  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_readback.py --trace-workload
              (fx_gather_candidates_kernel: 20 launches of 800 records, then 20 x 16 launches for 22 440 records)
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from frenetix_motion_planner_amd import _abi  # noqa: E402
from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls  # noqa: E402
from tests.fixtures import inputs_from_fixture, load_golden  # noqa: E402
from tests.handler_fixture import evaluate, make_handler  # noqa: E402


def stats(us):
    us = np.asarray(us) * 1e6
    return dict(p50_us=float(np.median(us)), p5_us=float(np.percentile(us, 5)), p95_us=float(np.percentile(us, 95)), reps=len(us))


def record_bytes(inp):
    return 8 * (_abi.FX_NUM_PLANES * inp.n_samples + 13 + len(inp.cost_names) + 4)


def read_pair(eng, ids, reps, reps_loop, label):
    """batched call and single-read loop, alternating"""
    inp = eng._inputs[0]
    for _ in range(3):
        eng.candidates(ids)
        [eng.candidate(int(g)) for g in ids[:64]]
    tb, tl = [], []
    every = max(1, reps // max(reps_loop, 1))
    for r in range(reps):
        t0 = time.perf_counter()
        eng.candidates(ids)
        tb.append(time.perf_counter() - t0)
        if r % every == 0 and len(tl) < reps_loop:
            t0 = time.perf_counter()
            for g in ids:
                eng.candidate(int(g))
            tl.append(time.perf_counter() - t0)
    b, l = stats(tb), stats(tl)
    n_bytes = len(ids) * record_bytes(inp)
    chunks = -(-len(ids) // (_abi.FX_READ_CHUNK_BYTES // (record_bytes(inp) + 8)))
    print(json.dumps(dict(metric="read", step=label, n=len(ids), samples=inp.n_samples, record_bytes=record_bytes(inp), bytes=n_bytes,
                          chunks=chunks, batched=b, single_loop=l, speedup_p50=l["p50_us"] / b["p50_us"],
                          batched_host_gbps=n_bytes / b["p50_us"] / 1e3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--reps-big", type=int, default=200)
    ap.add_argument("--trace-workload", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    h, matrix = make_handler(None)
    h.reset_Trajectories()
    evaluate(h, matrix())
    eng = h.engine
    big = inputs_from_fixture(load_golden("arc_hv_l4_horizon5_prod_obs8"), build_obstacle_hulls)
    if a.trace_workload:
        ids = np.arange(800, dtype=np.int64)
        for _ in range(20):
            eng.candidates(ids)
        with FrenetEngine(max_candidates=big.n_candidates, max_steps=big.N, max_pred_steps=max(64, big.N + 2)) as e2:
            e2.plan_step(big)
            ids = np.arange(big.n_candidates, dtype=np.int64)
            for _ in range(20):
                e2.candidates(ids)
        print(json.dumps(dict(metric="bytes", records_800=800 * record_bytes(eng._inputs[0]),
                              records_22440=big.n_candidates * record_bytes(big),
                              per_chunk_big=_abi.FX_READ_CHUNK_BYTES // (record_bytes(big) + 8))), flush=True)
        h.engine.close()
        return
    for n in (6, 8, 64, 800):
        ids = np.sort(rng.choice(800, n, replace=False)).astype(np.int64)
        read_pair(eng, ids, a.reps, a.reps, "matrix800")
    with FrenetEngine(max_candidates=big.n_candidates, max_steps=big.N, max_pred_steps=max(64, big.N + 2)) as e2:
        e2.plan_step(big)
        read_pair(e2, np.sort(rng.choice(big.n_candidates, 800, replace=False)).astype(np.int64), a.reps, a.reps, "l4_horizon5")
        read_pair(e2, np.arange(big.n_candidates, dtype=np.int64), a.reps, a.reps_big, "l4_horizon5")
    # reset_Trajectories() with k live samples: a fresh evaluated step per repetition, only the reset is timed
    m = matrix()
    for k in (0, 6, 800):
        ts = []
        for r in range(a.reps + 5):
            evaluate(h, m)
            trajs = h.get_sorted_trajectories()
            kept = trajs[:k] if k < 800 else trajs
            del trajs
            gc.collect()
            gc.disable()
            t0 = time.perf_counter()
            h.reset_Trajectories()
            t1 = time.perf_counter()
            gc.enable()
            if r >= 5:
                ts.append(t1 - t0)
            del kept
        print(json.dumps(dict(metric="reset_Trajectories", live_samples=k, **stats(ts))), flush=True)
    h.engine.close()


if __name__ == "__main__":
    main()
