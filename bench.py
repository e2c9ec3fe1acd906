#!/usr/bin/env python3
"""bench.py -- headline benchmark of the Frenet sampling-and-evaluation hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

Default workload (BASELINE.json configs[2], the largest single-GPU configuration): single agent, dense grid 19 x 51 x 52 =
50 388 candidates x 31 samples (30-step horizon), 20 predicted obstacles (obstacle 0 a slow lead vehicle so that the cheapest
candidates collide): prediction cost + OBB collision stage, constant-curvature reference with 400 knots, default cost
weights, SoA TrajectoryBundle materialised ("Mode B": every candidate's 14 planes written to HBM, as the reference's default
`draw_traj_set` configuration keeps them).  `--workload config2` drops the obstacles; `--select-only` drops the bundle
("Mode A").

A step = one plan step of the hot path: evaluation kernel + selection kernel + (N > 1) ONE RCCL all-gather of the per-GPU
survivors, finished on the host (the winner is in host memory when the step ends).  The contract's timed region -- `value`,
`ms_per_step` -- runs K such steps with the inputs resident in HBM.  For N > 1 the global grid is N x 50 388 candidates (the
velocity range is sampled N times denser) and each rank evaluates a contiguous shard: weak scaling.

A plain run does only that: set-up, preheat, W warm-up steps, the K timed steps, the line.  What needs runs of its own is
measured with `--full` only: a second region of K steps that feeds every step a NEW ego state and NEW predictions from host
buffers (fx_update_step: tables re-packed into the pinned staging block, one host-to-device copy, evaluation, result):
`plan_step_p50_ms` / `value_with_upload` are that PCIe-inclusive plan step; and in the same run, same JSON line (`north_star`),
the target workload of BASELINE.json -- 1 005 100 candidates x 31 samples x 20 obstacles, select-only (FP64-issue-bound:
executed-work roofline) and 1 005 100 x 31 with the 3.49 GB bundle materialised (HBM-bound).

`python bench.py --gpus N` without a launcher starts its own N ranks (torch.distributed.run on 127.0.0.1) before anything
touches the GPU and relays rank 0's line.

Other workloads (parity-test configurations of BASELINE.json, measured on request):
  --workload config1   the ego of ZAM_Tjunction-1_42_T-1, default sampling (630 candidates), 5 predicted obstacles;
  --workload config5   "synthetic stress": `--agents-per-gpu` (default 32 = 256 agents / 8 GPUs) agents per GPU x
                       39 x 51 x 52 = 103 428 candidates x 51 samples (5 s horizon), 20 predicted obstacles per agent,
                       select-only, one batched launch per step, per-agent top-32 survivors all-gathered (agent sharding:
                       N GPUs carry N x 32 agents -- weak scaling);
  --workload config4   multi-agent ZAM_Tjunction closed loop (5 agents, dense 19 x 23 x 23(+1) grid per agent, materialised
                       bundle, collision stage against the other agents' plans): a step = one simulation step of every agent.

Timing.  Before the W warm-up steps the engine runs untimed steps for `--preheat` seconds (default 0.3; reported as
`clock_preheat_s`): an idle GPU spends its first milliseconds at a lower clock and W = 5 steps are half a millisecond.  The
K timed steps carry no instrumentation; the kernel durations of `roofline` come from an instrumented repeat of the same K
steps (HIP events attached to every evaluation launch), because an instrumented launch costs 6 - 9 us of host time
(`--full`).

`--dump-outputs DIR` writes, after the timed steps, what the last timed step computed -- the arrays a caller of that path
receives -- as DIR/<name>.npy (float64; flag words and indices are exact in float64): the winner record, every candidate's
cost and flag word, the raw partial costs, and the planes of a fixed seeded sample of candidates plus the winner (the whole
bundle of config 3 is 175 MB).  The inputs are seeded, so two builds run with the same arguments can be compared array by
array.  Rank 0 writes: with several ranks the candidate arrays are rank 0's shard, the winner record leads with the global
winner.

Prints ONE JSON line (rank 0).  `value` = candidates evaluated by all ranks / wall time of the K timed steps.
"""
import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s peak
BYTES_PER_CAND_MODE_A = 40     # 3 x 8 B read + 8 B cost + 4 B flags + 4 B index
GRID = (19, 51, 51)            # n_t, n_v, n_d (+ d0) -> 50 388
NORTH_STAR_GRID = (19, 230, 229)  # 19 x 230 x 230 (d0 added) = 1 005 100 candidates
FP64_VALU_PEAK_TFLOPS = 78.6   # MI355X_MICROARCH.md: FP64 vector peak (256 CUs x 4 SIMDs x 16 lanes x 2 flop x 2.4 GHz)
LEAD_GAP = 25.0                # obstacle 0 is a slow lead vehicle 25 m ahead (the cheapest candidates collide)
STRESS_GRID = (39, 51, 51)     # config 5: T = 1.1 .. 4.9 (39) x 51 x 51 (+ d0), 5 s horizon
PROFILE_SUMMARY = os.path.join(ROOT, "profiles", "r6", "summary.json")  # rocprofv3 summaries of these commands (tools/collect_profiles.sh)
UPSTREAM_NOTE = "upstream OpenMP C++ handler (frenetix 0.4.0): not run -- not installable offline, not in the reference tree"


def bundle_bytes_per_candidate(n_samples):
    return 14 * n_samples * 8  # 3 472 B at 31 samples


def profile_summary():
    try:
        return json.load(open(PROFILE_SUMMARY))
    except (OSError, ValueError):
        return {}


def kernel_names(info, bundle, obstacles_fused, extra=False):
    """Names (as rocprofv3 prints them) of the evaluation kernels a step launched, from fx_step_info_ex: the walk and -- when
    the obstacle stage ran on its own -- the obstacle kernel."""
    b = lambda v: "true" if v else "false"
    if info["grid_kernel"]:
        walk = (f"fx_eval_grid_kernel<{info['lanes_per_candidate']}, {b(bundle)}, {b(obstacles_fused)}, {info['waves_per_simd']}, "
                f"{b(info['wave_split'])}>")
    else:
        walk = f"fx_eval_kernel<{info['lanes_per_candidate']}, {b(bundle)}, {b(obstacles_fused)}, {b(extra)}, {info['waves_per_simd']}>"
    obst = (f"fx_obstacle_kernel<{info['obstacle_steps_per_item']}, 4, {b(info.get('obstacle_workgroup_waves', 0) > 0)}>"
            if info.get("obstacle_kernel") else None)
    return walk, obst


def kernel_pmc(section, kernel):
    """Per-launch PMC means of `kernel` in `section` of the tracked summary -- None unless the summary holds THIS kernel (a
    changed tuning launches another specialisation: its counters would describe a different kernel)."""
    for name, pmc in profile_summary().get(section, {}).get("kernels", {}).items():
        if kernel and kernel in name:
            return pmc
    return None


def executed_fp64_flops(section, kernel):
    """FP64 flops one launch EXECUTES, from the tracked PMC summary of the same workload and kernel: 64 lanes x (ADD + MUL +
    2 FMA + transcendental) wave-instructions (SQ_INSTS_VALU_*_F64; an upper bound in that partially masked instructions count
    whole).  None when the summary does not hold this kernel."""
    pmc = kernel_pmc(section, kernel) or {}
    try:
        return 64.0 * (pmc["SQ_INSTS_VALU_ADD_F64"] + pmc["SQ_INSTS_VALU_MUL_F64"] + 2.0 * pmc["SQ_INSTS_VALU_FMA_F64"] +
                       pmc["SQ_INSTS_VALU_TRANS_F64"])
    except KeyError:
        return None


def pmc_traffic(section, kernel):
    """HBM bytes per launch from the tracked PMC passes (separate --pmc runs): WRITE_SIZE [KiB] x 1024 + FETCH_SIZE [KiB] x
    1024 x 2 (MI355X_MICROARCH.md: gfx950 FETCH_SIZE reports half of the bytes read)."""
    pmc = kernel_pmc(section, kernel) or {}
    try:
        return pmc["WRITE_SIZE"] * 1024.0 + 2.0 * pmc["FETCH_SIZE"] * 1024.0
    except KeyError:
        return None


def fp64_roofline(section, kernel, kernel_ms, units=None):
    """Executed-work view of one kernel: FP64 flops per launch from the tracked PMC summary of the SAME kernel over the live
    HIP-event duration.  When the summary holds another specialisation (the tuning changed since the passes were taken) no
    fraction is printed at all -- `flops_source` says "stale" -- rather than one that describes a different kernel."""
    fl = executed_fp64_flops(section, kernel)
    if fl is not None and units is not None:
        # the tracked passes ran `units_per_launch` units (agents) per launch; this run launches `units`
        per = profile_summary().get(section, {}).get("units_per_launch")
        fl = fl * units / per if per else None
    if fl is None:
        return {"bound": "fp64_valu", "achieved": None, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": None, "traffic": None,
                "flops_per_launch": None, "kernel": kernel, "avg_launch_ms": kernel_ms,
                "flops_source": f"stale: {os.path.relpath(PROFILE_SUMMARY, ROOT)} has no PMC section for {kernel} -- no executed-work figure"}
    tf = fl / (kernel_ms * 1e-3) / 1e12
    return {"bound": "fp64_valu", "achieved": tf, "peak": FP64_VALU_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP64_VALU_PEAK_TFLOPS,
            "traffic": pmc_traffic(section, kernel), "flops_per_launch": fl, "kernel": kernel, "avg_launch_ms": kernel_ms,
            "flops_source": "executed FP64 instructions of this kernel (SQ_INSTS_VALU_*_F64 x 64 lanes), " + os.path.relpath(PROFILE_SUMMARY, ROOT)}


def make_workload(args, world, grid=GRID, n_obst=None, select_only=None):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    if n_obst is None:
        n_obst = 20 if args.workload == "config3" else 0
    if select_only is None:
        select_only = args.select_only
    grid = (grid[0], grid[1] * world, grid[2])
    return synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=grid, n_obstacles=n_obst, n_pred=30, lead_gap=LEAD_GAP,
                                 write_bundle=not select_only, write_costmap=not select_only,
                                 draw_traj_set=False, kinematic_debug=False,
                                 hull_builder=build_obstacle_hulls if n_obst else None)


DUMP_LIMIT_BYTES = 64 << 20
DUMP_SAMPLE = 2048             # candidates whose planes --dump-outputs writes (fixed seed)
RESULT_FIELDS = ("best_index", "best_cost", "n_returned", "n_feasible", "n_infeasible", "n_collisions", "feasible_percentage")


def result_record(res):
    """One step result (dict or FxResult view) as floats in RESULT_FIELDS order (the global winner first with several ranks)."""
    return [float(res.get("global_best_index", res["best_index"])), float(res.get("global_best_cost", res["best_cost"]))] + \
           [float(res[k]) for k in RESULT_FIELDS]


def sample_index(n, k, best=-1):
    """A fixed seeded sample of k of n candidates, sorted, with the winner added."""
    idx = np.random.default_rng(20240601).choice(n, min(n, k), replace=False)
    return np.union1d(idx, np.array([best] if best >= 0 else [], dtype=idx.dtype))


def engine_outputs(eng, inp, res, agent=0):
    """What one agent's step left on the device for its caller: costs and flag words of every candidate, the raw partial
    costs, and the planes [n, 14, S] of a seeded sample of candidates and the winner (when the bundle is materialised)."""
    from frenetix_motion_planner_amd import _abi
    cost, flags = eng.costs(agent)
    out = {"result": result_record(res), "reason_hist": res["reason_hist"], "cost": cost, "flags": flags}
    if inp.write_costmap and len(inp.cost_names):
        out["costmap"] = eng.costmap(agent)
    if inp.write_bundle:
        idx = sample_index(inp.n_candidates, DUMP_SAMPLE, int(res["best_index"]))
        out["bundle_sample_index"] = idx
        out["bundle_sample"] = np.stack([eng.plane(p, agent)[:, idx] for p in range(_abi.FX_NUM_PLANES)]).transpose(2, 0, 1)
    return out


def stress_outputs(eng, agents, res, surv):
    """Config 5: every agent's result record, the gathered per-agent top-k survivors, and the costs and flag words of a seeded
    sample of each agent's candidates (all of them would be 26 MB per 32 agents and array)."""
    idx = sample_index(agents[0].n_candidates, 4 * DUMP_SAMPLE)
    cf = [eng.costs(a) for a in range(len(agents))]
    out = {"result": [result_record(r) for r in res], "cost_sample": [c[idx] for c, _ in cf],
           "flags_sample": [f[idx] for _, f in cf], "sample_index": idx}
    if surv is not None:
        out["survivor_cost"], out["survivor_index"] = surv
    return out


def dump_outputs(directory, arrays):
    """--dump-outputs: DIR/<name>.npy, float64."""
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(directory, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(directory, k + ".npy"), a)


def _host_threads():
    """Host threads this process can really run at once: the affinity mask capped by the cgroup CPU quota (the GPU box
    shows 256 CPUs but grants 16 cores' worth of time)."""
    try:
        n = max(1, len(os.sched_getaffinity(0)))
    except AttributeError:
        n = max(1, os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = max(1, min(n, int(quota + 0.5)))
    return n


def _time_oracle(inp, seconds, n_threads):
    """(trajectories/s, passes, seconds): whole passes over the candidate set; with threads the team lives for a batch of
    passes (sized from a probe so that the leg takes about `seconds`)."""
    from oracle import oracle
    C = inp.n_candidates
    oracle.plan_range(inp, 0, min(C, 2000))  # warm-up
    if n_threads <= 1:
        t0 = time.perf_counter()
        reps = 0
        while time.perf_counter() - t0 < seconds:
            oracle.plan_range(inp, 0, C)
            reps += 1
        dt = time.perf_counter() - t0
        return reps * C / dt, reps, dt
    t0 = time.perf_counter()
    oracle.plan_range(inp, 0, C, n_threads=n_threads, reps=2)
    probe = (time.perf_counter() - t0) / 2
    reps = int(max(4, min(2000, seconds / max(probe, 1e-4))))
    t0 = time.perf_counter()
    oracle.plan_range(inp, 0, C, n_threads=n_threads, reps=reps)
    dt = time.perf_counter() - t0
    return reps * C / dt, reps, dt


def cpu_baseline_of(inp, what):
    """The CPU oracle (scalar C restatement of the reference's algorithm) on the same workload, on this box's host
    cores: whole plan steps for ~8 s on every available core (pthreads over candidate chunks -- the stand-in for the
    upstream OpenMP handler, which is not installable offline) and ~5 s on one thread.  Reported, not optimised."""
    threads = _host_threads()
    one, reps1, dt1 = _time_oracle(inp, 5.0, 1)
    ref_py = None
    try:   # the reference's OWN Python path, timed where it can be imported (the build container): a committed record, data only
        import json as _json
        ref_py = _json.load(open(os.path.join(ROOT, "tests", "golden", "reference_python_timing.json")))
    except (OSError, ValueError):
        pass
    out = {"value": one, "unit": "trajectories/s", "cores": 1, "kind": "port", "reference_python": ref_py,
           "sample": f"{reps1} whole plan steps of {what} in {dt1:.1f} s, oracle/fx_oracle.c single thread",
           "cpu": _cpu_model(), "host_cores": os.cpu_count(), "upstream_handler": UPSTREAM_NOTE}
    if threads > 1:
        many, repsN, dtN = _time_oracle(inp, 8.0, threads)
        out.update({"value": many, "cores": threads, "single_thread_value": one,
                    "cpu_quota_cores": threads,
                    "sample": f"{repsN} whole plan steps of {what} in {dtN:.1f} s on {threads} threads (= the cores this "
                              f"process is granted) "
                              f"(oracle/fx_oracle.c, candidate chunks over pthreads); single thread: {reps1} steps in {dt1:.1f} s"})
    return out


def cpu_baseline(args):
    from frenetix_motion_planner_amd import synthetic
    from oracle import oracle
    n_obst = 20 if args.workload == "config3" else 0
    inp = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=GRID, n_obstacles=n_obst, n_pred=30, lead_gap=LEAD_GAP,
                                hull_builder=oracle.build_obstacle_hulls if n_obst else None)
    return cpu_baseline_of(inp, f"the same workload ({inp.n_candidates} candidates x {inp.n_samples} samples, {n_obst} obstacles)")


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (one per GPU, torch.distributed.run on
    127.0.0.1) BEFORE this process touches the GPU, relay their output, return their exit code.  (A process that has
    initialised the GPU must not be replaced by exec on this platform; a child process is always safe.)"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.run(cmd, env=env).returncode


def dry_launch(args, world, rank):
    """CPU-only check of the launch path: the ranks rendezvous over gloo, agree on the world size, rank 0 prints a line."""
    import torch
    import torch.distributed as dist
    # what every rank would work on (no engine, no GPU): the candidate shard of the default workload, the agent slice of config 5,
    # the (agent, part) items of config 4 -- gathered so that rank 0 can say whether the ranks' pieces cover the job exactly once
    from frenetix_motion_planner_amd.distributed import hybrid_assignment, shard_range
    C3 = 19 * 51 * 52 * max(world, 1)   # (make_workload: the velocity range sampled `world` times denser)
    b, n = shard_range(C3, rank, world)
    mine = [float(b), float(n), float(rank * args.agents_per_gpu), float(args.agents_per_gpu), float(len(hybrid_assignment(5, world)[rank]))]
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
        t = torch.tensor([1.0])
        dist.all_reduce(t)
        seen = int(t.item())
        rows = [torch.zeros(5, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(rows, torch.tensor(mine, dtype=torch.float64))
        rows = [r.tolist() for r in rows]
        dist.barrier()
        dist.destroy_process_group()
    else:
        seen, rows = 1, [mine]
    if rank == 0:
        edges = sorted((int(r[0]), int(r[0] + r[1])) for r in rows)
        covered = edges[0][0] == 0 and edges[-1][1] == C3 and all(edges[i][1] == edges[i + 1][0] for i in range(len(edges) - 1))
        agents = sorted(int(r[2]) for r in rows)
        print(json.dumps({"metric": "dry launch", "n_gpus": world, "ranks_seen": seen, "steps": args.steps, "warmup": args.warmup,
                          "workload": args.workload, "candidate_shards_cover_the_grid": bool(covered), "candidates_global": C3,
                          "config5_first_agents": agents, "config5_agents_global": int(world * args.agents_per_gpu),
                          "config4_items_per_rank": [int(r[4]) for r in rows]}))
    return 0


def perturbed_updates(eng, inp, n):
    """n plan-step updates around the workload's state: the ego a little further along the reference each time (new x_cl,
    new sampling values for the end velocities) and every predicted obstacle shifted along its track -- what a planner
    hands over from one step to the next.  Pre-built so that the timed loop measures the library, not NumPy."""
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    from frenetix_motion_planner_amd.problem import pack_predictions
    ups = []
    for j in range(n):
        x0_lon = np.array(inp.x0_lon) + np.array([0.05 * (j + 1), 0.01 * ((j % 3) - 1), 0.0])
        x0_lat = np.array(inp.x0_lat) + np.array([0.01 * ((j % 5) - 2), 0.0, 0.0])
        obstacles = None
        if inp.obstacles["K"] > 0 and getattr(inp, "predictions", None):
            preds = {}
            for k, pr in inp.predictions.items():
                q = dict(pr)
                step = np.array([np.cos(pr["orientation_list"][0]), np.sin(pr["orientation_list"][0])]) * 0.02 * (j + 1)
                q["pos_list"] = np.asarray(pr["pos_list"]) + step[None, :]
                preds[k] = q
            obstacles = pack_predictions(preds, inp.n_samples, build_obstacle_hulls)
        ups.append(eng.make_state_update(x0_lon=x0_lon, x0_lat=x0_lat, x0_orientation=inp.x0_orientation, v_des=inp.v_des,
                                         v_samp=np.asarray(inp.v_samp) + 1e-3 * (j % 4), obstacles=obstacles))
    return ups


def north_star(args, local_rank):
    """BASELINE.json's target workload in the same run: 1 005 100 x 31 x 20 obstacles (select-only), 1 005 100 x 31 with the
    bundle materialised, and both at once.  Kernel time from HIP events attached to every launch of a short timed region."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    out = {}
    # ... and the literal sentence of BASELINE.json's north star: the same million candidates WITH the 20 obstacles' prediction
    # cost and OBB collision check AND the SoA TrajectoryBundle in HBM, selection included
    for key, n_obst, select_only in (("obstacles_select_only", 20, True), ("bundle_no_obstacles", 0, False), ("bundle_obstacles", 20, False)):
        inp = make_workload(args, 1, grid=NORTH_STAR_GRID, n_obst=n_obst, select_only=select_only)
        C, S = inp.n_candidates, inp.n_samples
        eng = FrenetEngine(max_candidates=C + 64, max_steps=inp.N, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64,
                           device=local_rank)
        eng.set_timing("kernel", every=1)
        eng.upload(inp)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.3:  # a kernel after idle is timed at a lower clock
            eng.step_raw()
        n = 24
        ts = time.perf_counter()
        for _ in range(n):
            res = eng.step_raw()[0]
        step_ms = (time.perf_counter() - ts) / n * 1e3
        evalk, _ = eng.kernel_times(n)
        k_ms = float(np.mean(evalk))
        rec = {"workload": f"{C} candidates x {S} samples, {n_obst} predicted obstacles, "
                           f"{'select-only (Mode A)' if select_only else 'SoA TrajectoryBundle materialised (Mode B)'}",
               "candidates": C, "samples": S, "obstacles": n_obst, "eval_kernel_ms": k_ms, "step_ms": step_ms,
               "value": C / (step_ms * 1e-3), "launches_timed": int(len(evalk)),
               "winner": {"index": int(res.best_index), "cost": float(res.best_cost), "n_collisions": int(res.n_collisions)},
               "target": "< 10 ms on one MI355X"}
        info = eng.step_info()
        k_walk, _ = kernel_names(info, not select_only, bool(n_obst))
        rec["launch"] = info
        if select_only:
            rec["roofline"] = fp64_roofline("north_star_obstacles", k_walk, k_ms)
        elif n_obst:
            # both bounds: the 3.49 GB store stream of the bundle and the executed FP64 work of the fused obstacle stage
            alg = bundle_bytes_per_candidate(S) * C
            ach = alg / (k_ms * 1e-3) / 1e9
            rec["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                               "algorithmic_bytes_per_launch": alg, "traffic": pmc_traffic("north_star_bundle_obstacles", k_walk),
                               "kernel": k_walk, "note": "3.49 GB per launch: past the 256 MiB Infinity Cache"}
            rec["compute"] = fp64_roofline("north_star_bundle_obstacles", k_walk, k_ms)
        else:
            alg = bundle_bytes_per_candidate(S) * C
            ach = alg / (k_ms * 1e-3) / 1e9
            rec["roofline"] = {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                               "algorithmic_bytes_per_launch": alg, "traffic": pmc_traffic("north_star_bundle", k_walk),
                               "kernel": k_walk, "note": "3.49 GB per launch: past the 256 MiB Infinity Cache"}
        out[key] = rec
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", choices=["config1", "config2", "config3", "config4", "config5"],
                    default=os.environ.get("FX_BENCH_WORKLOAD", "config3"),
                    help="default: config3 (the configuration BASELINE.json's metric is quoted on), or $FX_BENCH_WORKLOAD -- a driver that "
                         "only passes --gpus / --steps / --warmup selects the agent-sharded workloads that way")
    ap.add_argument("--agents-per-gpu", type=int, default=32, help="config5: agents evaluated per GPU in one batched launch")
    ap.add_argument("--sampling-level", type=int, default=-1,
                    help="config4: reference sampling level of every agent instead of the dense 19 x 23 x 23 grid (4 -> 11 220 candidates)")
    ap.add_argument("--select-only", action="store_true", help="Mode A: no SoA bundle write")
    ap.add_argument("--topk", type=int, default=1, help="survivors per GPU in the exchange (1: the winner, no top-k kernel)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-north-star", action="store_true", help="skip the 1 M-candidate target workloads")
    ap.add_argument("--timing", choices=["stream", "kernel"], default="kernel",
                    help="HIP events around the evaluation kernel: attached to the kernel (hipExtLaunchKernel) or stream events")
    ap.add_argument("--timing-every", type=int, default=0,
                    help="attach the events to every n-th launch of the timed region (0: every launch below 64 steps, else every 8th)")
    ap.add_argument("--preheat", type=float, default=0.3,
                    help="seconds of untimed steps before the W warm-up steps (clock ramp of an idle GPU; 0 = none)")
    ap.add_argument("--dry-launch", action="store_true", help="CPU-only check of the multi-rank launch path (gloo)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: kernel times and rooflines, the host-fed plan step, the "
                         "north-star workloads, the CPU baseline, the multi-rank agent-sharding showcase, config 1's C++-style step")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed to DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.timing_every <= 0:
        args.timing_every = 1 if args.steps < 64 else 8

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))  # nothing has touched the GPU yet
    if args.dry_launch:
        sys.exit(dry_launch(args, world, rank))

    import torch
    import torch.distributed as dist

    if args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} but the launcher started {world} ranks", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible -- the engine has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    from frenetix_motion_planner_amd.distributed import ShardedEvaluator
    from frenetix_motion_planner_amd.engine import FrenetEngine

    if args.workload == "config1":
        return bench_scenario_step(args, world, rank, local_rank, torch, dist)
    if args.workload == "config5":
        return bench_stress(args, world, rank, local_rank, torch, dist)
    if args.workload == "config4":
        return bench_multiagent(args, world, rank, local_rank, torch, dist)

    inp = make_workload(args, world)
    C_global = inp.n_candidates_global
    from frenetix_motion_planner_amd.distributed import exit_on_timeout, verified_evaluator

    def prepare(eng_, ev_):
        ev_.shard(inp)
        eng_.upload(inp)

    # several ranks: the library-side survivor exchange is cross-checked once against the torch.distributed exchange of the same
    # step (untimed) and switched off everywhere if the two differ; `exchange` in the line says which one the timed steps used
    eng, ev, exchange_note = exit_on_timeout(verified_evaluator, lambda: FrenetEngine(
        max_candidates=C_global // world + 64, max_steps=inp.N, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64,
        device=local_rank), args.topk, prepare)
    C_local = inp.n_candidates
    S = inp.n_samples
    n_obst = int(inp.obstacles["K"])

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def step():
        # inputs are resident: upload happened once; a step re-runs evaluation + selection (+ survivor exchange); with several
        # ranks a peer that never joins ends this process with an error after the time bound instead of hanging the job
        return ev.step_enqueued() if world == 1 else exit_on_timeout(ev.step_enqueued)

    preheat(step, args.preheat, world, 1.2e-4)
    for _ in range(args.warmup):
        res = step()
    barrier()
    lat = []
    gc_was = gc.isenabled()
    gc.disable()   # (as timeit does: a collector pass inside K = 20 steps of 85 us is a 20 - 50 us outlier in the mean)
    try:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ts = time.perf_counter()
            res = step()
            lat.append(time.perf_counter() - ts)
        barrier()
        elapsed = time.perf_counter() - t0
    finally:
        if gc_was:
            gc.enable()
    if os.environ.get("FX_BENCH_LAT") and rank == 0:   # the K host latencies themselves (microseconds), for looking at outliers
        print("step latencies us:", " ".join(f"{x * 1e6:.1f}" for x in lat), file=sys.stderr)
    winner = {"index": int(res.get("global_best_index", res["best_index"])),
              "cost": float(res.get("global_best_cost", res["best_cost"])), "n_feasible_local": int(res["n_feasible"]),
              "n_collisions": int(res["n_collisions"])}
    dump_error = None
    if args.dump_outputs and rank == 0:   # (`res` views the engine's result buffer: read before any further step)
        try:
            dump_outputs(args.dump_outputs, engine_outputs(eng, inp, res))
        except Exception as e:   # raised once every rank knows (below): no peer is left waiting inside a collective
            dump_error = e
    rank_ms = [elapsed / args.steps * 1e3]
    if world > 1:
        # every rank's time and whether rank 0's dump failed, in one all-gather
        t = torch.tensor([elapsed, float(dump_error is not None)], dtype=torch.float64, device="cuda")
        allr = torch.empty(2 * world, dtype=torch.float64, device="cuda")
        dist.all_gather_into_tensor(allr, t)
        allr = allr.cpu().view(world, 2)
        rank_ms = [float(x) / args.steps * 1e3 for x in allr[:, 0].tolist()]
        elapsed = float(allr[:, 0].max().item())   # the contract's time: MAX over the ranks
        if allr[:, 1].any() and dump_error is None:
            dist.destroy_process_group()
            sys.exit("bench.py: --dump-outputs failed on rank 0")
    if dump_error is not None:
        if world > 1:
            dist.destroy_process_group()
        raise dump_error
    ms_per_step = elapsed / args.steps * 1e3
    line = {
        "metric": "candidate trajectories/sec (30-step horizon)",
        "value": C_global * args.steps / elapsed, "unit": "trajectories/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "clock_preheat_s": args.preheat,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": f"BASELINE {args.workload}: single agent, {C_local} candidates/GPU x {S} samples "
                               f"({GRID[0]}x{GRID[1]}x{GRID[2] + 1} grid per GPU), "
                               f"{'20 predicted obstacles (prediction cost + OBB collision)' if n_obst else 'no obstacles'}, "
                               f"{'select-only (Mode A)' if args.select_only else 'SoA TrajectoryBundle materialised (Mode B)'}",
                   "candidates_global": C_global, "candidates_per_gpu": C_local, "samples": S,
                   "reference_knots": int(inp.coordinate_system.ref_pos.shape[0]), "obstacles": n_obst,
                   "parallelism": f"candidate-shard x{world}, all-gather top-{args.topk}" if world > 1 else "single GPU",
                   "exchange": exchange_note},
        # how stable the timed region was: K steps are a few milliseconds of wall time
        "ms_per_step_min": float(np.min(lat) * 1e3), "ms_per_step_stdev": float(np.std(lat) * 1e3),
        "steps_timed_wall_ms": elapsed * 1e3,
        "resident_step_p50_ms": float(np.percentile(lat, 50) * 1e3), "resident_step_p95_ms": float(np.percentile(lat, 95) * 1e3),
        "ms_per_step_rank_min": min(rank_ms), "ms_per_step_rank_max": max(rank_ms), "ms_per_step_ranks": rank_ms,
        "winner": winner,
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(line), flush=True)
        eng.close()
        if world > 1:
            dist.destroy_process_group()
        return

    # Kernel durations: the same K steps once more, now with HIP events attached to EVERY evaluation launch (an instrumented
    # launch costs 6 - 9 us of host time, which has no place in `value`; the events live in a ring and are read afterwards)
    eng.set_timing(args.timing, every=1)
    n_timed = min(256, args.steps)
    for _ in range(n_timed):
        step()
    barrier()
    evalk, kern = eng.kernel_times(n_timed)
    obstk = eng.obstacle_kernel_times(n_timed)
    info = eng.step_info()
    comm = None
    try:
        if world > 1 and ev.uses_library_exchange():
            comm = eng.comm_info()
    except Exception:
        comm = None

    # the same K steps fed from host buffers: every step a new ego state and new predictions (single-rank steps; with
    # N > 1 every rank does the same update, the exchange is the one above)
    eng.set_timing("off")
    ups = perturbed_updates(eng, inp, 8)
    upd_step = (lambda u: eng.update_step_raw(u)) if world == 1 else (lambda u: (eng.update_state(u), step()))
    for j in range(max(4, args.warmup // 2)):
        upd_step(ups[j % len(ups)])
    barrier()
    lat_u = []
    tu = time.perf_counter()
    for j in range(args.steps):
        ts = time.perf_counter()
        upd_step(ups[j % len(ups)])
        lat_u.append(time.perf_counter() - ts)
    barrier()
    elapsed_u = time.perf_counter() - tu
    if world > 1:
        t = torch.tensor([elapsed_u], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed_u = float(t.item())

    # device-throughput figure: K evaluations enqueued back to back, one sync (informational)
    eng.upload(inp)
    barrier()
    tq = time.perf_counter()
    for _ in range(args.steps):
        eng.evaluate()
    eng.finish()
    torch.cuda.synchronize()
    pipelined = time.perf_counter() - tq
    eng.close()

    # Several ranks, default workload: BASELINE config 5 -- 32 agents per GPU, agent sharding, ONE per-agent top-k all-gather per step --
    # is measured by the same ranks in the same run (`agent_sharding`).  Config 3's 85 us step puts a latency-bound all-gather on every
    # step (DESIGN.md 6 predicts ~0.75 weak-scaling efficiency at 8 GPUs), config 5's 3.5 ms step hides it (~0.99).  With several ranks
    # it runs AFTER the headline line has been printed and reports on stderr (and into gpurun_out/ where that exists): a failure that
    # is local to one rank (out of memory, an FxError on one device) leaves its peers inside the showcase's collectives until the
    # process group's timeout -- the contract's line must not depend on that.  FX_BENCH_SHOWCASE=0 switches it off everywhere,
    # "force" runs it with one rank too, inside the line (the GPU test-suite).
    sc_env = os.environ.get("FX_BENCH_SHOWCASE", "1")

    def run_showcase():
        keep_env = os.environ.get("FX_EXCHANGE")
        os.environ["FX_EXCHANGE"] = "torch"
        try:
            sub = argparse.Namespace(**vars(args))
            sub.steps, sub.warmup, sub.preheat, sub.no_cpu_baseline = min(args.steps, 50), min(args.warmup, 5), 0.0, True
            sub.dump_outputs = None
            sc = bench_stress(sub, world, rank, local_rank, torch, dist, emit=False)
            if rank != 0 or sc is None:
                return None
            return {k: sc[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step", "scaling", "config",
                                       "plan_step_p50_ms", "eval_kernel_ms", "agents_with_winner")}
        except Exception as e:
            return {"error": f"{type(e).__name__}: {e}"} if rank == 0 else None
        finally:
            if keep_env is None:
                os.environ.pop("FX_EXCHANGE", None)
            else:
                os.environ["FX_EXCHANGE"] = keep_env

    showcase = run_showcase() if (world == 1 and sc_env == "force") else None

    if rank == 0:
        walk_ms = float(np.mean(evalk))
        obst_ms = float(np.mean(obstk)) if info["obstacle_kernel"] else 0.0
        eval_ms = walk_ms + obst_ms
        per_cand = BYTES_PER_CAND_MODE_A if args.select_only else bundle_bytes_per_candidate(S)
        alg_bytes = per_cand * C_local
        achieved = alg_bytes / (walk_ms * 1e-3) / 1e9
        section = f"{args.workload}_{'modeA' if args.select_only else 'modeB'}"
        k_walk, k_obst = kernel_names(info, not args.select_only, bool(n_obst) and not info["obstacle_kernel"])
        timing_note = ("HIP events attached to every evaluation launch (hipExtLaunchKernel start/stop) of an instrumented "
                       "repeat of the timed steps, same process and inputs; the timed region itself carries no events"
                       if args.timing == "kernel" else "stream events around every launch of an instrumented repeat of the timed steps")
        traffic = pmc_traffic(section, k_walk) if world == 1 else None
        hbm = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
               "traffic": traffic, "traffic_source": os.path.relpath(PROFILE_SUMMARY, ROOT) if traffic else None,
               "algorithmic_bytes_per_launch": alg_bytes, "bytes_per_candidate": per_cand,
               "kernel": k_walk + ("" if n_obst else " (evaluation + fused selection)"), "avg_launch_ms": walk_ms,
               "launches_timed": int(len(evalk)), "timing": timing_note}
        kernels = [hbm]
        if n_obst and info["obstacle_kernel"]:
            # the step's obstacle stage ran as its own kernel: the walk is the store stream (bytes), the obstacle kernel FP64 issue
            ob = fp64_roofline(section, k_obst, obst_ms)
            ob.update({"launches_timed": int(len(obstk)), "timing": timing_note})
            kernels.append(ob)
            # the dominant kernel of the step; the two take the same 40 us on config 3 -- within 5 % the walk stands (the bound
            # BASELINE.json names: HBM), so that the line does not flip between runs; `kernels` carries both either way
            roofline = ob if obst_ms > 1.05 * walk_ms else hbm
        elif n_obst:
            # fused obstacle stage: FP64-issue-bound, executed work of this kernel against the FP64 vector peak
            roofline = fp64_roofline(section, k_walk, walk_ms)
            roofline.update({"launches_timed": int(len(evalk)), "timing": timing_note})
            kernels = [roofline]
        else:
            roofline = hbm
        out = dict(line, **{
            # the step a planner really takes (new ego state + predictions from host buffers every step), next to `value`
            "plan_step_value": C_global * args.steps / elapsed_u, "plan_step_ms": elapsed_u / args.steps * 1e3,
            "plan_step_p50_ms": float(np.percentile(lat_u, 50) * 1e3), "plan_step_p95_ms": float(np.percentile(lat_u, 95) * 1e3),
            "plan_step_note": "plan_step_* = the step fed a new ego state and new predictions from host buffers every time "
                              "(fx_update_step: re-packed tables, one host-to-device copy, evaluation, result on the host); "
                              "resident_step_* and value = inputs resident in HBM",
            "with_upload_ms_per_step": elapsed_u / args.steps * 1e3, "value_with_upload": C_global * args.steps / elapsed_u,
            "device_ms_per_step": float(np.mean(kern)), "eval_kernel_ms": eval_ms, "walk_kernel_ms": walk_ms,
            "obstacle_kernel_ms": obst_ms, "launch": info,
            "pipelined_value": C_global * args.steps / pipelined,
            # a scaling record checks itself: the ranks RCCL reports for the library's communicator (ncclCommCount; the torch
            # group's size when the exchange ran through torch.distributed) and every rank's own time for the K steps
            "rccl_ranks": (comm["rccl_ranks"] if comm and comm["rccl_ranks"] > 0 else world) if world > 1 else 1,
            "roofline": roofline,
            "kernels": kernels,
        })
        if showcase is not None:
            out["agent_sharding"] = showcase
        if n_obst:
            out["roofline_hbm"] = hbm
        # the whole step against the HBM roofline: algorithmic bytes of the step over the STEP's wall time (launch gaps, obstacle
        # kernel and selection included) -- a figure that cannot move by re-partitioning the work between kernels
        step_gbs = alg_bytes / (ms_per_step * 1e-3) / 1e9
        out["roofline_step"] = {"bound": "hbm", "achieved": step_gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": step_gbs / HBM_PEAK_GBS,
                                "algorithmic_bytes_per_step": alg_bytes, "ms_per_step": ms_per_step,
                                "note": "algorithmic bytes of one step / ms_per_step (resident inputs, whole step incl. obstacle kernel, "
                                        "selection and launch gaps)"}
        if world == 1 and not args.no_north_star:
            out["north_star"] = north_star(args, local_rank)
        if not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(args)
        elif world == 1:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if world > 1 and sc_env != "0":   # behind the headline (see above): stderr + gpurun_out/agent_sharding_<N>.json
        sc = run_showcase()
        if rank == 0 and sc is not None:
            print("[bench] agent_sharding " + json.dumps(sc), file=sys.stderr, flush=True)
            try:
                if os.path.isdir(os.path.join(ROOT, "gpurun_out")):
                    with open(os.path.join(ROOT, "gpurun_out", f"agent_sharding_{world}.json"), "w") as f:
                        json.dump(sc, f)
            except OSError:
                pass
    if world > 1:
        dist.destroy_process_group()


def preheat(step, seconds, world=1, est_step_s=1e-4):
    """Untimed steps for about `seconds` before the W warm-up steps: a GPU that has been idle runs its first milliseconds at a
    lower clock (measured: the first 2 ms after start-up are 5 - 10 % slower), and W = 5 steps are 0.5 ms.  With several ranks
    the steps contain a collective, so every rank runs the same COUNT of steps (seconds / the workload's nominal step time)."""
    if seconds <= 0:
        return 0
    if world > 1:
        n = max(1, int(seconds / est_step_s))
        for _ in range(n):
            step()
        return n
    t0 = time.perf_counter()
    n = 0
    while time.perf_counter() - t0 < seconds:
        step()
        n += 1
    return n


def _timed(args, world, dist, torch, step, est_step_s=1e-4):
    """W warm-up steps, then exactly K steps between barrier + synchronize; max over ranks.  Returns (elapsed s, per-step
    host latencies)."""
    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
    if est_step_s:   # a closed-loop simulation is not preheated: every step advances its state
        preheat(step, args.preheat, world, est_step_s)
    for _ in range(args.warmup):
        step()
    barrier()
    lat = []
    gc_was = gc.isenabled()
    gc.disable()   # (as timeit does)
    try:
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ts = time.perf_counter()
            step()
            lat.append(time.perf_counter() - ts)
        barrier()
        elapsed = time.perf_counter() - t0
    finally:
        if gc_was:
            gc.enable()
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    return elapsed, lat


def bench_stress(args, world, rank, local_rank, torch, dist, emit=True):
    """BASELINE config 5: agents sharded over the GPUs, one batched launch per step, per-agent top-k gather.
    emit=False: called from the default workload's multi-rank run -- rank 0 returns the record instead of printing it, the
    process group stays up."""
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.distributed import ShardedEvaluator
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    n_local = args.agents_per_gpu
    k = 32 if args.topk == 1 else args.topk
    agents = synthetic.stress_agents(n_local, grid=STRESS_GRID, first_agent=rank * n_local, hull_builder=build_obstacle_hulls)
    C_local = sum(a.n_candidates for a in agents)
    S, K = agents[0].n_samples, int(agents[0].obstacles["K"])
    from frenetix_motion_planner_amd.distributed import exit_on_timeout, verified_evaluator

    def prepare(eng_, ev_):
        ev_.setup_agents(n_local)
        eng_.upload(agents)

    eng, ev, exchange_note = exit_on_timeout(verified_evaluator, lambda: FrenetEngine(
        max_candidates=C_local + 64 * n_local, max_steps=agents[0].N, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64,
        device=local_rank, max_agents=n_local), k, prepare)
    eng.set_timing(args.timing, every=args.timing_every)
    last = {}

    def step():
        last["res"], last["surv"] = ev.step_agents_enqueued() if world == 1 else exit_on_timeout(ev.step_agents_enqueued)

    elapsed, lat = _timed(args, world, dist, torch, step, 5e-3)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, stress_outputs(eng, agents, last["res"], last["surv"]))
    n_timed = min(256, (args.steps + args.timing_every - 1) // args.timing_every)
    evalk, kern = eng.kernel_times(n_timed)
    obstk = eng.obstacle_kernel_times(n_timed)
    info = eng.step_info()
    if rank == 0:
        C_global = C_local * world  # every rank carries the same number of candidates (same grid per agent)
        eval_ms = float(np.mean(evalk))
        alg_bytes = BYTES_PER_CAND_MODE_A * C_local
        achieved = alg_bytes / (eval_ms * 1e-3) / 1e9
        k_walk, _ = kernel_names(info, False, True)
        # executed FP64 work of THIS kernel from the tracked PMC pass (the planning figure of SURVEY 8(d) prices a full
        # axis test per (obstacle, step) although the broad phase skips nearly all of them: it is not used here)
        compute = fp64_roofline("config5_modeA", k_walk, eval_ms, units=n_local)
        res = last["res"]
        out = {
            "metric": "candidate trajectories/sec (50-step horizon, 20 obstacles per agent)",
            "value": C_global * args.steps / elapsed, "unit": "trajectories/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"BASELINE config5 (synthetic stress): {n_local} agents/GPU x {agents[0].n_candidates} candidates x "
                                   f"{S} samples, {K} predicted obstacles per agent (prediction cost + OBB collision), select-only "
                                   f"(Mode A), one batched launch per step, top-{k} survivors per agent",
                       "agents_global": n_local * world, "agents_per_gpu": n_local, "candidates_global": C_global,
                       "candidates_per_gpu": C_local, "samples": S, "obstacles": K,
                       "parallelism": f"agent-shard x{world}, all-gather of per-agent top-{k}" if world > 1 else "single GPU",
                       "exchange": exchange_note},
            "plan_step_p50_ms": float(np.percentile(lat, 50) * 1e3), "plan_step_p95_ms": float(np.percentile(lat, 95) * 1e3),
            "device_ms_per_step": float(np.mean(kern)), "eval_kernel_ms": eval_ms,
            "agents_with_winner": int(sum(r["best_index"] >= 0 for r in res)),
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": None, "kernel": k_walk + " (batched over agents)",
                         "algorithmic_bytes_per_launch": alg_bytes, "bytes_per_candidate": BYTES_PER_CAND_MODE_A,
                         "avg_launch_ms": eval_ms, "launches_timed": int(len(evalk)),
                         "note": "select-only writes 12 B per candidate: this workload is FP64-issue-bound, see `compute`"},
            "compute": compute, "launch": info,
        }
        if args.full and not args.no_cpu_baseline and world == 1:
            from oracle import oracle
            one = synthetic.stress_agents(1, grid=STRESS_GRID, hull_builder=oracle.build_obstacle_hulls)[0]
            out["cpu_baseline"] = cpu_baseline_of(one, f"agent 0 ({one.n_candidates} candidates x {S} samples, {K} obstacles)")
        if emit:
            print(json.dumps(out))
    eng.close()
    if not emit:
        return out if rank == 0 else None   # (`out` exists on rank 0)
    if world > 1:
        dist.destroy_process_group()


def bench_scenario_step(args, world, rank, local_rank, torch, dist):
    """BASELINE config 1 on the engine: the ego of ZAM_Tjunction-1_42_T-1, default sampling (level 2: 630 candidates x 31
    samples), the scenario's five cars as predicted obstacles, debug flag set of the reference's default configuration
    (bundle materialised, every candidate evaluated), collision stage.  A step = one plan step with resident inputs."""
    from frenetix_motion_planner_amd import commonroad_xml as crx
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from frenetix_motion_planner_amd.frenet_interface import FrenetPlannerInterfaceHip
    sc = crx.read_scenario_json(os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json"))
    itf = FrenetPlannerInterfaceHip(60000, sc, sc.planning_problems[60000], device=local_rank)
    itf.update_planner(None, sc.ground_truth_predictions(0, 30))
    inp = itf.begin_step()
    eng = FrenetEngine(max_candidates=4096, max_steps=inp.N, max_ref_knots=4096, max_obstacles=32, max_pred_steps=64, device=local_rank)
    eng.set_timing(args.timing, every=args.timing_every)
    eng.upload(inp)
    last = {}

    def step():
        eng.evaluate()
        last["res"] = eng.finish()[0]

    elapsed, lat = _timed(args, world, dist, torch, step, 5e-5)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, engine_outputs(eng, inp, last["res"]))
    n_timed = min(256, (args.steps + args.timing_every - 1) // args.timing_every)
    evalk, kern = eng.kernel_times(n_timed)
    obstk = eng.obstacle_kernel_times(n_timed)
    info = eng.step_info()
    # "630 candidates Python-style (800 with the C++-style unions {3.0}, {s'0}, {d0} -- report both)": the same
    # step in the form the reference's C++ adapter hands over, a C x 13 sampling matrix (reactive_planner_cpp.py:228-253)
    cpp_style = None
    res630 = dict(last["res"])
    if world == 1 and args.full:
        import copy
        from frenetix_motion_planner_amd.sampling import generate_sampling_matrix
        t = np.union1d(inp.t_samp, [inp.N * inp.dt]); v = np.union1d(inp.v_samp, [inp.x0_lon[1]]); d = np.union1d(inp.d_samp, [inp.x0_lat[0]])
        inp800 = copy.copy(inp)
        inp800.t_samp = inp800.v_samp = inp800.d_samp = None
        inp800.sampling_matrix = generate_sampling_matrix(
            t0_range=0.0, t1_range=t, s0_range=inp.x0_lon[0], ss0_range=inp.x0_lon[1], sss0_range=inp.x0_lon[2], ss1_range=v,
            sss1_range=0.0, d0_range=inp.x0_lat[0], dd0_range=inp.x0_lat[1], ddd0_range=inp.x0_lat[2], d1_range=d, dd1_range=0.0,
            ddd1_range=0.0)
        inp800.__post_init__()
        eng.upload(inp800)
        e800, lat800 = _timed(args, world, dist, torch, step, 5e-5)
        ev800, _ = eng.kernel_times(n_timed)
        cpp_style = {"candidates": int(inp800.n_candidates), "form": "C x 13 sampling matrix (generic kernel)",
                     "ms_per_step": e800 / args.steps * 1e3, "value": inp800.n_candidates * args.steps / e800,
                     "plan_step_p50_ms": float(np.percentile(lat800, 50) * 1e3), "eval_kernel_ms": float(np.mean(ev800)),
                     "winner": {"index": int(last["res"]["best_index"]), "cost": float(last["res"]["best_cost"])}}
    if rank == 0:
        C, S = inp.n_candidates, inp.n_samples
        eval_ms = float(np.mean(evalk))
        alg = bundle_bytes_per_candidate(S) * C
        out = {
            "metric": "candidate trajectories/sec (30-step horizon)", "value": C * args.steps / elapsed, "unit": "trajectories/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
            "data": "ZAM_Tjunction-1_42_T-1 (scenario fixture): ego planning problem, ground-truth predictions of the five cars",
            "config": {"workload": f"BASELINE config1: ZAM_Tjunction-1_42_T-1 single agent, default sampling level 2 ({C} candidates x {S} "
                                   "samples), 5 predicted obstacles, draw_traj_set / kinematic_debug as in debug.yaml, bundle materialised",
                       "candidates": C, "samples": S, "obstacles": int(inp.obstacles["K"]), "parallelism": "single GPU"},
            "plan_step_p50_ms": float(np.percentile(lat, 50) * 1e3), "plan_step_p95_ms": float(np.percentile(lat, 95) * 1e3),
            "device_ms_per_step": float(np.mean(kern)), "eval_kernel_ms": eval_ms,
            "winner": {"index": int(res630["best_index"]), "cost": float(res630["best_cost"]),
                       "n_feasible": int(res630["n_feasible"]), "n_collisions": int(res630["n_collisions"])},
            "roofline": {"bound": "hbm", "achieved": alg / (eval_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": alg / (eval_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None, "algorithmic_bytes_per_launch": alg,
                         "avg_launch_ms": eval_ms, "launches_timed": int(len(evalk)),
                         "note": "630 candidates = 10 waves: the step is launch-latency-bound, not bandwidth-bound"},
            "reference_python_path": "about 1.2e3 trajectories/s on one core (measured in the build container, BASELINE.md section 3)",
        }
        out["cpp_style_800"] = cpp_style
        if args.full and not args.no_cpu_baseline and world == 1:
            from oracle import oracle
            from frenetix_motion_planner_amd.problem import pack_predictions
            inp.obstacles = pack_predictions(inp.predictions if hasattr(inp, "predictions") and inp.predictions else
                                             sc.ground_truth_predictions(0, 30), S, oracle.build_obstacle_hulls)
            out["cpu_baseline"] = cpu_baseline_of(inp, f"the same plan step ({C} candidates x {S} samples, 5 obstacles)")
        print(json.dumps(out))
    eng.close()
    itf.close()
    if world > 1:
        dist.destroy_process_group()


def bench_multiagent(args, world, rank, local_rank, torch, dist):
    """BASELINE config 4: closed-loop multi-agent ZAM_Tjunction; agents dealt to the GPUs by distributed.hybrid_assignment (whole
    agents round-robin, or -- fewer agents than GPUs -- every GPU one part of an agent's candidates)."""
    from frenetix_motion_planner_amd import commonroad_xml as crx
    from frenetix_motion_planner_amd.multiagent import MultiAgentSimulation
    from frenetix_motion_planner_amd.reactive_planner import PlannerConfig
    sc = crx.read_scenario_json(os.path.join(ROOT, "tests", "golden", "ZAM_Tjunction-1_42_T-1.scenario.json"))
    lvl = args.sampling_level
    if lvl >= 0:
        cfg = PlannerConfig(sampling_min=lvl, sampling_max=lvl + 1)
    else:  # dense 19 x 23 x 23 (+ the current d) grid per agent
        cfg = PlannerConfig(sampling_min=0, sampling_max=1, dense_grid=(19, 23, 23))
    sim = MultiAgentSimulation(sc, config=cfg, device=local_rank, freeze_gc=True)
    counts = {"cands": 0, "batch_ms": []}

    from frenetix_motion_planner_amd.distributed import exit_on_timeout

    def step():
        before = sim.batch.launches
        sim.step() if world == 1 else exit_on_timeout(sim.step)
        if sim.batch.launches > before:
            counts["batch_ms"].append(sim.batch.last_batch_ms)

    elapsed, lat = _timed(args, world, dist, torch, step, None)
    if args.dump_outputs and rank == 0:   # the planned trajectories of every agent [agents, S, fields], identical on every rank
        dump_outputs(args.dump_outputs, {"plans": sim.plans})
    if rank == 0:
        n_agents = len(sim.agent_ids)
        ls = sim.batch.agents[0].planner.last_step
        per_agent = ls.inputs.n_candidates_global if ls else 0
        plan_steps = len(counts["batch_ms"])
        out = {
            "metric": "candidate trajectories/sec (30-step horizon), closed-loop multi-agent simulation",
            "value": per_agent * n_agents * plan_steps / elapsed, "unit": "trajectories/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "strong",
            "vs_baseline": None, "dtype": "f64", "data": "ZAM_Tjunction-1_42_T-1 (scenario fixture), agents' own plans as predictions",
            "config": {"workload": f"BASELINE config4: multi-agent ZAM_Tjunction, {n_agents} agents x {per_agent} candidates x 31 samples "
                                   f"({'sampling level ' + str(lvl) if lvl >= 0 else 'dense 19 x 23 x 23(+1) grid'}), bundle materialised, collision stage; a step = one simulation step "
                                   "(replanning every 3rd step)",
                       "agents": n_agents, "candidates_per_agent": per_agent, "plan_steps_timed": plan_steps,
                       "pipeline_groups": len(sim.batch.engines),
                       "parallelism": ("single GPU" if world == 1 else
                                       (f"{n_agents} agents over {world} GPUs: every GPU one contiguous part of an agent's candidates "
                                        f"({[len([1 for it in sim.items for k, _, _ in it if k == a]) for a in range(n_agents)]} parts), "
                                        "winners merged in one all-gather, one all-gather of the plans per step") if sim.split else
                                       f"agent round-robin x{world}, one all-gather of the plans per step"),
                       "items_per_gpu": [len(it) for it in sim.items]},
            "sim_step_p50_ms": float(np.percentile(lat, 50) * 1e3), "sim_step_p95_ms": float(np.percentile(lat, 95) * 1e3),
            "batched_plan_launch_ms": float(np.median(counts["batch_ms"])) if plan_steps else None,
            "escalations": sim.batch.escalations,
        }
        print(json.dumps(out))
    sim.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
