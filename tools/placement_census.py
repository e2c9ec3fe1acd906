#!/usr/bin/env python3
"""Placement census of the split step's two big launches: where the hardware puts their waves.

Runs tools/micro/placement (stand-in kernels with the launch shape, registers and LDS of config 3's walk and obstacle kernel; built
with hipcc if the binary is missing) and prints, per kernel: workgroups per CU, waves per SIMD, which wave indices of a ten-wave
workgroup share a SIMD, how the two workgroups of a CU stack, and duration / end time by waves-per-SIMD class.

usage: placement_census.py [--walk-lds B] [--obst-lds B] [--walk-iters N] [--obst-iters N] [--reps N] [--weights w0,..,w9] [--perm HEX]
                           [--obst-waves N] [--csv FILE] [--out FILE]
--weights gives the ten chunks of the obstacle stand-in their own chain lengths, --perm maps wave w to chunk (HEX >> 4 w) & 15: what
placing chunks by weight gains on the measured placement, before anything is built into the real kernel.  --obst-waves launches the
obstacle stand-in with more than ten waves per workgroup (the extra ones only wait at the barrier): how the live waves then stack.
The LDS sizes default to what the launch policy gives config 3 on this device (fx_step_info_ex), else to the recorded 39 936 / 34 000 B.
"""
import argparse, collections, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "micro", "placement")


def config3_lds():
    """(walk LDS, obstacle-kernel launch LDS) of config 3 from a real context"""
    sys.path.insert(0, ROOT)
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, n_pred=30, grid=(19, 51, 51), n_obstacles=20,
                                lead_gap=25.0)
    with FrenetEngine(max_candidates=inp.n_candidates + 64, max_steps=inp.N) as eng:
        eng.upload(inp)
        eng.evaluate(); eng.finish()
        i = eng.step_info()
    waves = i["obstacle_workgroup_waves"]
    return i["lds_bytes"], (waves * (i["obstacle_lds_bytes"] + 64 * 8 + 8) + 15) // 16 * 16, i


def hist(counter):
    return "  ".join(f"{k}: {v}" for k, v in sorted(counter.items()))


def peak(intervals):
    """largest number of intervals open at once"""
    ev = sorted([(a, 1) for a, _ in intervals] + [(b, -1) for _, b in intervals], key=lambda e: (e[0], e[1]))
    n = best = 0
    for _, d in ev:
        n += d
        best = max(best, n)
    return best


def census(name, rows, n_cus, waves_per_wg, out):
    P = lambda *a: print(*a, file=out)
    P(f"== {name}: {len({r['wg'] for r in rows})} workgroups x {waves_per_wg} waves, {len(rows)} wave records ==")
    t0_max, t1_min, t1_max = max(r["t0"] for r in rows), min(r["t1"] for r in rows), max(r["t1"] for r in rows)
    P(f"last start {t0_max / 1e3:.2f} us, first end {t1_min / 1e3:.2f} us, last end {t1_max / 1e3:.2f} us "
      f"({'every wave was resident at once' if t0_max < t1_min else 'NOT all resident at once: later rounds counted by peak overlap'})")
    by_cu, by_simd, by_wg = collections.defaultdict(list), collections.defaultdict(list), collections.defaultdict(list)
    for r in rows:
        cu = (r["xcc"], r["se"], r["sh"], r["cu"])
        by_cu[cu].append(r); by_simd[cu + (r["simd"],)].append(r); by_wg[r["wg"]].append(r)
    P(f"XCCs {sorted({k[0] for k in by_cu})}, SEs {sorted({k[1] for k in by_cu})}, distinct CUs used {len(by_cu)} of {n_cus}")
    # workgroups per CU: every workgroup the CU ever held, and the most it held at once
    wg_total = collections.Counter(len({r["wg"] for r in v}) for v in by_cu.values())
    wg_total[0] = n_cus - len(by_cu)
    wg_peak = collections.Counter()
    cu_peak = {}
    for cu, v in by_cu.items():
        spans = {}
        for r in v:
            a, b = spans.get(r["wg"], (r["t0"], r["t1"]))
            spans[r["wg"]] = (min(a, r["t0"]), max(b, r["t1"]))
        cu_peak[cu] = peak(list(spans.values()))
        wg_peak[cu_peak[cu]] += 1
    wg_peak[0] = n_cus - len(by_cu)
    P(f"workgroups per CU (CUs with n workgroups over the launch): {hist(wg_total)}")
    P(f"workgroups per CU (resident at once, peak):                {hist(wg_peak)}")
    simd_peak = {k: peak([(r["t0"], r["t1"]) for r in v]) for k, v in by_simd.items()}
    sp = collections.Counter(simd_peak.values())
    sp[0] = 4 * n_cus - len(by_simd)
    P(f"waves per SIMD (resident at once, peak; SIMDs with n waves): {hist(sp)}")
    # which wave indices of a workgroup share a SIMD
    pat = collections.Counter()
    one_cu = 0
    for wg, v in by_wg.items():
        one_cu += len({(r["xcc"], r["se"], r["sh"], r["cu"]) for r in v}) == 1
        groups = collections.defaultdict(list)
        for r in v:
            groups[r["simd"]].append(r["wave"])
        pat[" / ".join(",".join(map(str, sorted(g))) for g in sorted(groups.values(), key=lambda g: min(g)))] += 1
    P(f"workgroups whose waves share one CU: {one_cu} of {len(by_wg)}")
    P("wave indices sharing a SIMD (pattern: workgroups):")
    for k, n in pat.most_common(8):
        P(f"    {k}: {n}")
    if len(pat) > 8:
        P(f"    ... {len(pat) - 8} more patterns, {sum(pat.values()) - sum(n for _, n in pat.most_common(8))} workgroups")
    # how the workgroups of a CU stack on its SIMDs
    stack = collections.Counter()
    for cu, v in by_cu.items():
        n_wg = len({r["wg"] for r in v})
        per = tuple(sorted((simd_peak.get(cu + (s,), 0) for s in range(4)), reverse=True))
        stack[(n_wg, per)] += 1
    P("waves on the four SIMDs of a CU, by workgroups on the CU (n workgroups, (sorted waves per SIMD)): CUs")
    for (n_wg, per), n in sorted(stack.items()):
        P(f"    {n_wg} workgroup(s) {'-'.join(map(str, per))}: {n}")
    # duration and end by the wave's SIMD load
    P("by waves-per-SIMD class of the wave's own SIMD: waves, mean / max duration us, mean / max end us")
    cls = collections.defaultdict(list)
    for k, v in by_simd.items():
        for r in v:
            cls[simd_peak[k]].append(r)
    for k in sorted(cls):
        d = [(r["t1"] - r["t0"]) / 1e3 for r in cls[k]]
        e = [r["t1"] / 1e3 for r in cls[k]]
        P(f"    {k} wave(s) on the SIMD: {len(d):5d} waves, duration {sum(d) / len(d):6.2f} / {max(d):6.2f}, end {sum(e) / len(e):6.2f} / {max(e):6.2f}")
    P("by workgroups on the wave's CU (peak): waves, mean / max duration us, mean / max end us")
    cls = collections.defaultdict(list)
    for cu, v in by_cu.items():
        cls[cu_peak[cu]].extend(v)
    for k in sorted(cls):
        d = [(r["t1"] - r["t0"]) / 1e3 for r in cls[k]]
        e = [r["t1"] / 1e3 for r in cls[k]]
        P(f"    {k} workgroup(s) on the CU: {len(d):5d} waves, duration {sum(d) / len(d):6.2f} / {max(d):6.2f}, end {sum(e) / len(e):6.2f} / {max(e):6.2f}")
    P("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walk-lds", type=int); ap.add_argument("--obst-lds", type=int)
    ap.add_argument("--walk-iters", type=int, default=800); ap.add_argument("--obst-iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5); ap.add_argument("--weights"); ap.add_argument("--perm", default="9876543210")
    ap.add_argument("--obst-waves", type=int, default=10)
    ap.add_argument("--csv"); ap.add_argument("--out")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    note = "defaults"
    if a.walk_lds is None or a.obst_lds is None:
        try:
            wl, ol, info = config3_lds()
            note = f"from config 3's step info {info}"
        except Exception as e:   # no library / no device: the recorded sizes
            wl, ol, note = 39936, 34000, f"recorded sizes ({type(e).__name__}: {e})"
        a.walk_lds = a.walk_lds or wl; a.obst_lds = a.obst_lds or ol
    if not os.path.exists(BIN):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-o", BIN, BIN + ".hip"], check=True)
    p = subprocess.run([BIN, str(a.walk_lds), str(a.obst_lds), str(a.walk_iters), str(a.obst_iters), str(a.reps),
                        a.weights or ",".join([str(a.obst_iters)] * 10), a.perm, str(a.obst_waves)], capture_output=True, text=True, timeout=120)
    if p.returncode:
        sys.exit(f"placement failed ({p.returncode}): {p.stderr[-2000:]}")
    if a.csv:
        open(a.csv, "w").write(p.stdout)
    rows, n_cus, events, times = collections.defaultdict(list), 256, {}, {}
    for line in p.stdout.splitlines():
        if line.startswith("# device"):
            n_cus = int(line.split()[-1])
        if line.startswith("# times"):
            times[line.split()[2]] = f"min {line.split()[4]} / median {line.split()[6]} us of {a.reps}"
        if line.startswith("# kernel"):
            events[line.split()[2]] = float(line.split()[-1])
        if line.startswith("#") or not line.strip():
            continue
        f = line.split(",")
        rows[f[0]].append(dict(zip(("wg", "wave", "xcc", "se", "sh", "cu", "simd", "slot", "t0", "t1"), map(int, f[1:]))))
    print(f"placement census: walk LDS {a.walk_lds} B, obstacle LDS {a.obst_lds} B ({note}); FMA chain {a.walk_iters} x 8 / {a.obst_iters} x 8; "
          f"{n_cus} CUs; kernel time by events: " + ", ".join(f"{k} {v:.1f} us ({times.get(k, '')})" for k, v in events.items()), file=out)
    if a.weights or a.perm != "9876543210" or a.obst_waves != 10:
        print(f"obstacle stand-in: chain lengths x 8 of chunks 0..9 = {a.weights or a.obst_iters}, wave -> chunk constant {a.perm}, "
              f"{a.obst_waves} waves per workgroup launched", file=out)
    print("", file=out)
    census("walk stand-in (394 x 256 lanes, 164 VGPRs)", rows["walk"], n_cus, 4, out)
    census("obstacle stand-in (788 x 640 lanes, 503 live, 74 VGPRs)", rows["obstacle"], n_cus, 10, out)


if __name__ == "__main__":
    main()
