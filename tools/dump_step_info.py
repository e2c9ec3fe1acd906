#!/usr/bin/env python3
"""The launch policy's decisions, recorded: for every row of a fixed table of plan steps -- sizes either side of every threshold,
every force, batches, every refusal -- upload, evaluate once and write fx_step_info_ex's 16 numbers (or the refusal's error
code and message) to JSON, next to what of the problems the policy reads.  tests/test_launch_policy.py holds csrc/fx_policy.h
to the committed recording (profiles/policy/step_info_parent.json) without a GPU, tests/test_launch_policy_gpu.py a real context.

    python tools/dump_step_info.py OUT.json [COMMIT]

The file keeps every row as its differences from the defaults and every distinct agent once (pack / unpack).
"""
import copy
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BIG = (20, 100, 100)   # at least 196 608 candidates: a shard of it pins an agent's candidate count exactly
CAPS = dict(max_candidates=197000, max_steps=50, max_ref_knots=1024, max_obstacles=80, max_pred_steps=64)
FORCE0 = dict(G=0, wpe=0, variant=0, block=0, mapping=0, obst_stage=0, obst_CH=0, fused=1, store=0, step_kernel=0, step_kernel_CH=0)
WINDOWED = {"acceleration": 1.0, "distance_to_reference_path": 1.0, "velocity_offset": 1.0, "prediction": 1.0}


def agent(C=None, grid=BIG, K=0, bundle=True, **kw):
    """one agent of a row: `C` candidates as a shard of `grid` (None: the whole grid), K obstacles, with / without the bundle"""
    return dict(C=C, grid=tuple(grid), K=K, bundle=bundle, **kw)


ENV0 = dict(FX_LDS_PAD=0, FX_OBST_WG=-1)   # the experiment knobs a row may set in the environment (-1: unset)


def case(name, agents, package=False, caps=None, patch=None, env=None, **force):
    """patch: fields of the first agent's FxProblem overwritten behind PlanInputs.as_struct (what Python would not build)"""
    assert set(force) <= set(FORCE0), force
    agents = agents if isinstance(agents, list) else [agents]
    return dict(name=name, agents=agents, package=package, caps=dict(CAPS, max_agents=len(agents), **(caps or {})),
                force=dict(FORCE0, **force), patch=patch or {}, env=dict(ENV0, **(env or {})))


def table():
    rows = []
    # candidate counts either side of every wave-count threshold of the lanes-per-candidate rule
    for waves in (31, 32, 99, 100, 199, 200, 3071, 3072):
        for K, bundle in ((0, False), (0, True), (5, False), (20, False), (5, True), (20, True)):
            rows.append(case(f"waves_{waves}_K{K}_{'bundle' if bundle else 'select'}", agent(64 * waves, K=K, bundle=bundle)))
    small = dict(grid=(5, 9, 14))   # 675 candidates: a planner-sized step
    for K in (0, 64, 65):
        rows.append(case(f"K_{K}", agent(K=K, **small)))
        rows.append(case(f"K_{K}_12800", agent(12800, K=K)))
    for K in (0, 5):
        rows.append(case(f"road_boundary_K{K}", agent(K=K, road_half_width=4.0, **small)))
        rows.append(case(f"road_boundary_K{K}_12800", agent(12800, K=K, road_half_width=4.0)))
        rows.append(case(f"windowed_K{K}", agent(K=K, cost_weights=WINDOWED, **small)))
        rows.append(case(f"windowed_K{K}_12800", agent(12800, K=K, cost_weights=WINDOWED)))
        rows.append(case(f"matrix_K{K}", agent(K=K, as_matrix=True, **small)))
        rows.append(case(f"matrix_K{K}_G4", agent(K=K, as_matrix=True, **small), G=4))
        rows.append(case(f"matrix_K{K}_G8_S51", agent(K=K, as_matrix=True, horizon=5.0, n_pred=50, **small), G=8))
    # few lateral samples per pair: many longitudinal rows per workgroup, up to no workgroup size that fits
    for nD in (1, 3):
        for S, hz in ((31, 3.0), (51, 5.0)):
            a = agent(K=5, grid=(10, 63, 8), nD=nD, horizon=hz, n_pred=int(hz * 10))
            for G in (0, 1, 2, 4, 8):
                rows.append(case(f"nD{nD}_S{S}_G{G}", a, G=G))
            rows.append(case(f"nD{nD}_S{S}_G2_wave", a, G=2, mapping=2))
    for S, hz in ((31, 3.0), (51, 5.0)):
        for K in (0, 5, 20):
            rows.append(case(f"S{S}_K{K}", agent(K=K, horizon=hz, n_pred=int(hz * 10), **small), package=True))
            rows.append(case(f"S{S}_K{K}_12800", agent(12800, K=K, horizon=hz, n_pred=int(hz * 10))))
    for M in (60, 409, 3000):
        ref = dict(n_knots=M, spacing=2.0 if M == 60 else 0.5, s_knot=5 if M == 60 else 40)
        big = dict(max_ref_knots=3000)
        rows.append(case(f"M{M}", agent(K=5, **ref, **small), caps=big))
        rows.append(case(f"M{M}_generic_G4", agent(K=5, **ref, **small), caps=big, variant=1, G=4))
        rows.append(case(f"M{M}_12800", agent(12800, K=5, **ref), caps=big))
    # every force, alone
    for K in (0, 5):
        a630, a12800 = agent(K=K, **small), agent(12800, K=K)
        for G in (1, 2, 4, 8, 16, 32):
            rows.append(case(f"force_G{G}_K{K}", a630, G=G))
            rows.append(case(f"force_G{G}_K{K}_generic", a630, G=G, variant=1))
        for wpe in (2, 3, 4):
            rows.append(case(f"force_wpe{wpe}_K{K}", a630, wpe=wpe))
            rows.append(case(f"force_wpe{wpe}_K{K}_3072", agent(64 * 3072, K=K), wpe=wpe))
        for variant in (1, 2):
            rows.append(case(f"force_variant{variant}_K{K}", a630, variant=variant))
            rows.append(case(f"force_variant{variant}_K{K}_12800", a12800, variant=variant))
        for block in (64, 128, 256):
            rows.append(case(f"force_block{block}_K{K}", a630, block=block))
            rows.append(case(f"force_block{block}_K{K}_12800", a12800, block=block))
            rows.append(case(f"force_block{block}_K{K}_G4", a630, block=block, G=4))
        for mapping in (1, 2):
            rows.append(case(f"force_mapping{mapping}_K{K}", a630, mapping=mapping))
            rows.append(case(f"force_mapping{mapping}_K{K}_12800", a12800, mapping=mapping))
            rows.append(case(f"force_mapping{mapping}_K{K}_G4", a630, mapping=mapping, G=4))
            rows.append(case(f"force_mapping{mapping}_K{K}_G2_block128", a630, mapping=mapping, G=2, block=128))
        for fused in (0, 1, 2):
            rows.append(case(f"force_fused{fused}_K{K}", a630, fused=fused, package=True))
            rows.append(case(f"force_fused{fused}_K{K}_8192", agent(8192, K=K), fused=fused))
            rows.append(case(f"force_fused{fused}_K{K}_8193", agent(8193, K=K), fused=fused))
            rows.append(case(f"force_fused{fused}_K{K}_G1", a630, fused=fused, G=1))
        for store in (1, 2):
            for package in (False, True):
                rows.append(case(f"force_store{store}_K{K}_package{int(package)}", a630, store=store, package=package))
        rows.append(case(f"package_K{K}_12800", a12800, package=True))
        rows.append(case(f"package_K{K}_select_only", agent(K=K, bundle=False, **small), package=True))
    for stage in (1, 2):
        for CH in (0, 2, 3, 5):
            rows.append(case(f"obst_stage{stage}_CH{CH}", agent(K=5, **small), obst_stage=stage, obst_CH=CH))
            rows.append(case(f"obst_stage{stage}_CH{CH}_12800_S51", agent(12800, K=20, horizon=5.0, n_pred=50), obst_stage=stage, obst_CH=CH))
    rows.append(case("obst_stage2_CH5_K64_S51", agent(K=64, horizon=5.0, n_pred=50, **small), obst_stage=2, obst_CH=5))   # workgroup LDS over a CU's
    rows.append(case("obst_stage2_CH2_S51", agent(K=5, horizon=5.0, n_pred=50, **small), obst_stage=2, obst_CH=2))        # 25 chunks: single-wave items
    rows.append(case("obst_stage2_1025_tiles", agent(64 * 1025, K=5), obst_stage=2))
    rows.append(case("obst_stage2_1024_tiles", agent(64 * 1024, K=5), obst_stage=2))
    rows.append(case("obst_stage2_CH5_K64_S61", agent(K=64, horizon=6.0, n_pred=60, **small), caps=dict(max_steps=60), obst_stage=2, obst_CH=5))
    rows.append(case("obst_stage2_items_by_env", agent(K=5, **small), obst_stage=2, env=dict(FX_OBST_WG=0)))
    rows.append(case("obst_stage2_workgroups_by_env", agent(64 * 1025, K=5), obst_stage=2, env=dict(FX_OBST_WG=1)))
    rows.append(case("lds_pad_by_env", agent(K=5, **small), env=dict(FX_LDS_PAD=70000)))
    rows.append(case("no_hulls", agent(K=5, hulls=False, collision=False, **small), package=True, patch=dict(obs_hull=None, obs_nhull=None)))
    rows.append(case("no_hulls_12800", agent(12800, K=5, hulls=False, collision=False), patch=dict(obs_hull=None, obs_nhull=None)))
    rows.append(case("road_boundary_flag_without_pieces", agent(K=0, road_half_width=4.0, **small), patch=dict(n_bound=0)))
    rows.append(case("force_G1_mapping2", agent(K=5, **small), G=1, mapping=2))
    for name in ("jerk", "orientation_offset", "path_length"):
        rows.append(case(f"windowed_{name}", agent(K=0, cost_weights={name: 1.0, "velocity_offset": 1.0}, **small)))
    rows.append(case("windowed_lane_center_offset", agent(K=0, cost_weights={"lane_center_offset": 1.0, "velocity_offset": 1.0}, lanelets=(3.5, 60), **small)))
    rows.append(case("obst_stage2_no_collision", agent(K=5, collision=False, **small), obst_stage=2, package=True))
    # the forced decompositions of tests/test_hip_reference_vectors.py, on a step with predictions and on one without
    tuned = dict(G=2, variant=2, block=256, mapping=2)
    for K in (0, 5):
        a = agent(K=K, **small)
        rows.append(case(f"variant_wave_split_2_K{K}", a, **tuned))
        rows.append(case(f"variant_wave_split_2_block_128_K{K}", a, G=2, variant=2, block=128, mapping=2))
        rows.append(case(f"variant_wave_split_4_K{K}", a, G=4, variant=2, block=256, mapping=2))
        for CH in (0, 3, 5, 8):
            rows.append(case(f"one_launch_CH{CH}_K{K}", a, obst_stage=2, step_kernel=2, step_kernel_CH=CH, **tuned))
    rows.append(case("one_launch_package", agent(K=5, **small), obst_stage=2, step_kernel=2, package=True, **tuned))
    rows.append(case("one_launch_12800_K20_S51", agent(12800, K=20, horizon=5.0, n_pred=50), obst_stage=2, step_kernel=2, **tuned))
    rows.append(case("one_launch_write_back", agent(K=5, **small), obst_stage=2, step_kernel=2, store=1, **tuned))
    rows.append(case("one_launch_automatic_walk", agent(12800, K=5), step_kernel=2))
    rows.append(case("one_launch_walk_too_large", agent(64 * 3071, K=5), obst_stage=2, step_kernel=2, **tuned))
    rows.append(case("one_launch_fused_stage", agent(K=5, **small), obst_stage=1, step_kernel=2, **tuned))
    rows.append(case("one_launch_G4", agent(K=5, **small), obst_stage=2, step_kernel=2, **dict(tuned, G=4)))
    rows.append(case("one_launch_lane_split", agent(K=5, **small), obst_stage=2, step_kernel=2, **dict(tuned, mapping=1)))
    rows.append(case("one_launch_block128", agent(K=5, **small), obst_stage=2, step_kernel=2, **dict(tuned, block=128)))
    rows.append(case("one_launch_wpe3", agent(K=5, **small), obst_stage=2, step_kernel=2, wpe=3, **tuned))
    rows.append(case("step_kernel_off", agent(K=5, **small), obst_stage=2, step_kernel=1, **tuned))
    # batches
    mixed = [agent(K=5, **small), agent(K=0, **small), agent(1984, K=20), agent(K=5, grid=(3, 9, 10), horizon=5.0, n_pred=50),
             agent(K=0, bundle=False, **small), agent(K=5, bundle=False, **small), agent(2048, K=0), agent(K=20, grid=(3, 9, 10))]
    rows.append(case("batch_8_mixed", mixed))
    rows.append(case("batch_8_mixed_package", mixed, package=True))
    rows.append(case("batch_8_mixed_obst_stage2", [a for a in mixed if a["bundle"]], obst_stage=2))
    rows.append(case("batch_33", [agent(K=5 if a % 3 else 0, grid=(3, 9 + a % 4, 10)) for a in range(33)]))
    rows.append(case("batch_33_fused0", [agent(K=5 if a % 3 else 0, grid=(3, 9 + a % 4, 10)) for a in range(33)], fused=0))
    pair = [agent(K=5, **small), agent(K=0, **small)]
    rows.append(case("batch_with_and_without_obstacles", pair, obst_stage=2))
    rows.append(case("batch_with_and_without_obstacles_one_launch", pair, obst_stage=2, step_kernel=2, **tuned))
    rows.append(case("batch_2_one_launch", [agent(K=5, **small), agent(K=20, **small)], obst_stage=2, step_kernel=2, **tuned))
    rows.append(case("batch_2_12800_auto_split", [agent(6400, K=5), agent(6400, K=0)]))
    # every refusal: forced but not applicable ...
    rows.append(case("refuse_obst_kernel_no_bundle", agent(K=5, bundle=False, **small), obst_stage=2))
    rows.append(case("refuse_obst_kernel_K65", agent(K=65, **small), obst_stage=2))
    rows.append(case("refuse_obst_kernel_road_boundary", agent(K=5, road_half_width=4.0, **small), obst_stage=2))
    rows.append(case("refuse_obst_kernel_windowed", agent(K=5, cost_weights=WINDOWED, **small), obst_stage=2))
    rows.append(case("refuse_grid_windowed", agent(K=5, cost_weights=WINDOWED, **small), variant=2))
    rows.append(case("refuse_grid_matrix", agent(K=0, as_matrix=True, **small), variant=2))
    rows.append(case("refuse_grid_K65", agent(K=65, **small), variant=2))
    rows.append(case("refuse_grid_lds", agent(K=5, grid=(10, 63, 8), nD=1), variant=2, G=1))
    rows.append(case("refuse_wave_split_G8", agent(K=0, **small), G=8, mapping=2))
    rows.append(case("refuse_wave_split_block64", agent(K=0, **small), G=2, block=64, mapping=2))
    rows.append(case("refuse_wave_split_generic", agent(K=0, **small), G=2, variant=1, mapping=2))
    # ... and one capacity error of each kind
    rows.append(case("refuse_capacity_N", agent(K=0, **small), caps=dict(max_steps=29)))
    rows.append(case("refuse_capacity_M", agent(K=0, **small), caps=dict(max_ref_knots=399)))
    rows.append(case("refuse_capacity_K", agent(K=5, **small), caps=dict(max_obstacles=4)))
    rows.append(case("refuse_capacity_P", agent(K=5, **small), caps=dict(max_pred_steps=29)))
    rows.append(case("refuse_capacity_candidates", [agent(K=0, **small), agent(K=0, **small)], caps=dict(max_candidates=1000)))
    rows.append(case("refuse_capacity_generic_lds", agent(K=0, n_knots=3000, **small), caps=dict(max_ref_knots=3000), variant=1))
    rows.append(case("refuse_shard_end", agent(K=0, **small), patch=dict(shard_begin=650, shard_count=31)))
    rows.append(case("refuse_shard_begin", agent(K=0, **small), patch=dict(shard_begin=-1, shard_count=31)))
    rows.append(case("refuse_shard_count", agent(K=0, **small), patch=dict(shard_count=-1)))
    names = [r["name"] for r in rows]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return rows


_INPUTS = {}


def inputs_of(spec):
    """PlanInputs of one agent of a row (built once per distinct problem; the shard is set on a copy)"""
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    kw = {k: v for k, v in spec.items() if k not in ("C", "K", "bundle", "nD", "hulls")}
    key = json.dumps(dict(kw, K=spec["K"], bundle=spec["bundle"], nD=spec.get("nD"), hulls=spec.get("hulls", True)), sort_keys=True, default=str)
    if key not in _INPUTS:
        inp = synthetic.make_inputs(ref_kind="arc", n_obstacles=spec["K"], write_bundle=spec["bundle"], write_costmap=spec["bundle"],
                                    hull_builder=build_obstacle_hulls if spec["K"] and spec.get("hulls", True) else None, **kw)
        if spec.get("nD"):
            inp.d_samp = np.ascontiguousarray(inp.d_samp[:spec["nD"]])
        _INPUTS[key] = inp
    inp = copy.copy(_INPUTS[key])
    inp.shard = (0, spec["C"]) if spec["C"] else None
    return inp


def describe(p):
    """what of an FxProblem the launch policy reads"""
    return dict(N=p.N, M=p.M, K=p.K, P=p.P, mode=p.mode, nT=p.nT, nV=p.nV, nD=p.nD, n_rows=p.n_rows, matrix=int(bool(p.sampling_matrix)),
                shard_begin=p.shard_begin, shard_count=p.shard_count, cost_id=[p.cost_id[n] for n in range(p.n_cost)],
                n_bound=p.n_bound, have_hull=int(bool(p.obs_hull) and bool(p.obs_nhull)))


class Runner:
    """runs rows of the table on real contexts and returns what the library answered.  reuse: one context per distinct set of
    capacities instead of one per row (a recording takes a fresh context per row, so that no row can see an earlier one)"""

    def __init__(self, reuse=False):
        self.engines, self.reuse = {}, reuse

    def close(self):
        for e in self.engines.values():
            e.close()
        self.engines = {}

    def run(self, row):
        from frenetix_motion_planner_amd import _abi
        from frenetix_motion_planner_amd._lib import lib
        from frenetix_motion_planner_amd.engine import FrenetEngine
        caps, f = row["caps"], row["force"]
        key = tuple(sorted(caps.items()))
        if not self.reuse:
            self.close()
        if key not in self.engines:
            self.engines[key] = FrenetEngine(**caps)
        e = self.engines[key]
        e.set_tuning(f["G"], f["wpe"], f["variant"], f["block"], f["mapping"])
        e.set_obstacle_stage(f["obst_stage"], f["obst_CH"])
        e.set_fused_selection(f["fused"])
        e.set_store_mode(f["store"])
        e.set_step_kernel(f["step_kernel"], f["step_kernel_CH"])
        e.set_package(row["package"])
        batch = [inputs_of(s) for s in row["agents"]]
        arr = (_abi.FxProblem * len(batch))(*[b.as_struct() for b in batch])
        for k, v in row["patch"].items():
            setattr(arr[0], k, v)
        out = dict(name=row["name"], caps=caps, force=f, env=row["env"], package=int(row["package"]), agents=[describe(p) for p in arr])
        e._inputs, e._structs = batch, arr
        for k, v in row["env"].items():   # (the library reads them at upload / at evaluation)
            os.environ.pop(k, None)
            if v != ENV0[k]:
                os.environ[k] = str(v)
        try:
            rc = lib().fx_upload_batch(e._ctx, len(batch), arr)
            if rc:
                out["error"] = dict(code=rc, message=lib().fx_last_error().decode())
                return out

            def step():
                e.evaluate()
                v = np.zeros(16, np.int64)
                lib().fx_step_info_ex(e._ctx, v.ctypes.data)
                res = e.finish()
                v[15] &= ~0xff00   # how the bytes reached the device depends on the machine (large BAR)
                return [int(x) for x in v], res

            out["info"], res = step()
            if f["step_kernel"] == 2:
                # a second step of the same upload: the one-launch step sizes its obstacle items by the first one's costed candidates
                out["last_live"] = max(r["n_returned"] if b.draw_traj_set else r["n_feasible"] for r, b in zip(res, batch))
                out["info_second"], _ = step()
        finally:
            for k in row["env"]:
                os.environ.pop(k, None)
        v = out["info"]
        if f["step_kernel"] == 2:
            # what the device answers the one-launch step's sizing: workgroups it holds at once per (steps per item, LDS bytes)
            cap_fn = lib().fx_step_kernel_capacity
            cap_fn.argtypes, cap_fn.restype = [C.c_int, C.c_size_t, C.POINTER(C.c_int)], C.c_int
            K_max, occ = max(p.K for p in arr), {}
            for CH in (3, 5, 8):
                n = C.c_int(0)
                lds = max(int(v[9]), 4 * 8 * 6 * CH * max(K_max, 0))
                occ[str(CH)] = n.value if cap_fn(CH, lds, C.byref(n)) == 0 else 0
            out["occupancy"] = occ
        return out


AGENT0 = dict(N=30, M=400, K=0, P=0, mode=12, nT=5, nV=9, nD=15, n_rows=0, matrix=0, shard_begin=0, shard_count=0, cost_id=[2, 5, 6, 10],
              n_bound=0, have_hull=0)   # the plain 675-candidate agent with the bundle: the recording keeps what differs from it


def _diff(d, base):
    return {k: v for k, v in d.items() if v != base[k]}


def pack(rows, commit):
    """the recording as it is written: every row as its differences from the defaults, every distinct agent once"""
    agents, packed = [], []
    for r in rows:
        x = dict(name=r["name"], agents=[])
        for a in r["agents"]:
            if a not in agents:
                agents.append(a)
            x["agents"].append(agents.index(a))
        for key, base in (("caps", dict(CAPS, max_agents=len(r["agents"]))), ("force", FORCE0), ("env", ENV0)):
            if _diff(r[key], base):
                x[key] = _diff(r[key], base)
        x.update({k: r[k] for k in ("package", "info", "error", "last_live", "info_second", "occupancy") if k in r and (k != "package" or r[k])})
        packed.append(x)
    return dict(commit=commit, masked="bits 8-15 of info[15]", caps=CAPS, force=FORCE0, env=ENV0, agent=AGENT0,
                agents=[_diff(a, AGENT0) for a in agents], rows=packed)


def unpack(rec):
    """the rows of a recording in full, as Runner.run returns them"""
    agents = [dict(rec["agent"], **a) for a in rec["agents"]]
    rows = []
    for x in rec["rows"]:
        r = dict(x, agents=[agents[i] for i in x["agents"]], package=x.get("package", 0), force=dict(rec["force"], **x.get("force", {})),
                 env=dict(rec["env"], **x.get("env", {})), caps=dict(rec["caps"], max_agents=len(x["agents"]), **x.get("caps", {})))
        rows.append(r)
    return rows


def write(rec, out_path):
    with open(out_path, "w") as f:
        head = {k: v for k, v in rec.items() if k not in ("agents", "rows")}
        f.write(json.dumps(head)[:-1] + ',\n "agents": [\n')
        f.write(",\n".join("  " + json.dumps(a, separators=(",", ":")) for a in rec["agents"]))
        f.write('\n ],\n "rows": [\n')
        f.write(",\n".join("  " + json.dumps(x, separators=(",", ":")) for x in rec["rows"]))
        f.write("\n ]}\n")


def main():
    out_path = sys.argv[1]
    commit = sys.argv[2] if len(sys.argv) > 2 else "unknown"
    r = Runner()
    rows = [r.run(row) for row in table()]
    r.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    write(pack(rows, commit), out_path)
    n_err = sum("error" in x for x in rows)
    print(f"{len(rows)} rows ({n_err} refusals) -> {out_path}")


if __name__ == "__main__":
    main()
