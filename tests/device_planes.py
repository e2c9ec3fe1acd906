"""Arbitrary cost / flag planes for the reduction kernels, and the plain NumPy statement of what they must answer.

The top-k kernels read an agent's cost (f64) and flag (u32) planes afresh on every `topk()` call; `write_cost_flags` overwrites
them on the device after a finished step (pointers from `fx_device_views`, a host-to-device copy through the HIP runtime the
library has already loaded), so a test can show the kernels any plane: signs, infinities, NaN, ties by construction.  The selection
kernel reduces partials the evaluation kernel wrote, so its tests run real steps and only the references below are shared.

One rule, everywhere: the lexicographic (cost, index) order of Python's stable sort.  Importable without a GPU."""
import ctypes as C
import re

import numpy as np

from frenetix_motion_planner_amd import _abi

SEL, COL, BND = _abi.FX_FLAG_SELECTABLE, _abi.FX_FLAG_COLLISION, _abi.FX_FLAG_BOUNDARY

# ---- the sizes at which the kernels change their code path (tests/test_topk_planes.py::test_switch_sizes_follow_the_source
# derives each of them from the constants in csrc/ and fails when one moves) ----
TOPK_SLICES = 64                     # workgroups per agent of the slice stage
TOPK_WAVE_MAX_C = 131_072            # largest agent the one-wave slice kernel takes: 64 slices x 64 lanes x 32 register slots
TOPK_WAVE_MAX_K = 32                 # largest k of the one-wave merge: 64 lists x k <= 64 lanes x 32 LDS entries
SELECT_SLICES_MIN = 32               # slices of fx_select_kernel up to SELECT_SLICES_MIN * SELECT_PER_SLICE candidates
SELECT_PER_SLICE = 4_096             # the slice count doubles while slices * 4 096 < C
SELECT_PRELOAD = 8 * 256             # (flag, cost) pairs a workgroup requests at entry; a slice beyond them runs the second loop
SELECT_BATCH_WORKGROUPS = 2_048      # a batch halves its slices again while slices * n_agents exceeds this

TOPK_SIZES = (1, 63, 64, 65, 4_096, 4_097, 131_072, 131_073, 199_999)
TOPK_KS = (1, 31, 32, 33, 64)
SELECT_SIZES = (65_536, 65_537, 131_072, 131_073, 262_145)


def topk_slice_bounds(C_agent: int, s: int):
    """[lo, hi) of slice s of an agent's candidates in the top-k slice stage"""
    per = -(-C_agent // TOPK_SLICES)
    return min(C_agent, s * per), min(C_agent, (s + 1) * per)


def select_slices(C_max: int, n_agents: int = 1) -> int:
    """slices per agent of fx_select_kernel (fx_launch_select)"""
    s = SELECT_SLICES_MIN
    while s < 512 and s * SELECT_PER_SLICE < C_max:
        s *= 2
    while s > SELECT_SLICES_MIN and s * n_agents > SELECT_BATCH_WORKGROUPS:
        s //= 2
    return s


def select_slice_offset(C_agent: int, n_slices: int, g):
    """position of candidate(s) g within their slice of fx_select_kernel"""
    per = -(-C_agent // n_slices)
    return np.asarray(g) % per


def source_constants(csrc: str) -> dict:
    """The constants the sizes above follow from, read from the source text of csrc/."""
    import os
    kern = open(os.path.join(csrc, "fx_kernels.hip")).read()
    sel = open(os.path.join(csrc, "fx_select.h")).read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]

    out = dict(topk_slices=int(one(r"#define FX_TOPK_SLICES (\d+)", kern)), topk_r=int(one(r"#define FX_TOPK_R (\d+)", kern)),
               select_slices_min=int(one(r"#define FX_SELECT_SLICES_MIN (\d+)", sel)),
               select_slices_max=int(one(r"#define FX_SELECT_SLICES_MAX (\d+)", sel)),
               per_slice=int(one(r"\(int64_t\)slices \* (\d+) < max_candidates", kern)),
               batch_workgroups=int(one(r"\(int64_t\)slices \* n_agents > (\d+)", kern)))
    # the launcher's two conditions, as written
    assert one(r"if \(per (<=?) 64 \* FX_TOPK_R\)", kern) == "<="
    assert one(r"if \(FX_TOPK_SLICES \* k (<=?) 64 \* FX_TOPK_R\)", kern) == "<="
    assert "const int64_t per = (max_candidates + FX_TOPK_SLICES - 1) / FX_TOPK_SLICES;" in kern
    # the pre-load of fx_select_body: u < n pairs at a stride of the workgroup's lanes, the second loop behind them
    n_pre = {int(x) for x in re.findall(r"for \(int u = 0; u < (\d+); u\+\+\) \{\s*(?://[^\n]*\n\s*)?const int64_t gu = g0 \+ tid \+ u \* 256;", sel)}
    assert len(n_pre) == 1 and len(re.findall(r"gu = g0 \+ tid \+ u \* 256", sel)) == 2, n_pre
    out["preload_pairs"] = n_pre.pop()
    out["second_loop_start"] = tuple(int(x) for x in one(r"for \(int64_t g = g0 \+ tid \+ (\d+) \* (\d+); g < g1;", sel))
    assert one(r"__launch_bounds__\((\d+)\) void fx_select_kernel", sel) == "256"
    return out


# ---- writing the planes ----
_HIP = None


def _hip_runtime():
    """the HIP runtime libfxplan.so is linked against, as this process has it mapped"""
    global _HIP
    if _HIP is None:
        from frenetix_motion_planner_amd._lib import lib
        lib()
        paths = {line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}
        assert len(paths) == 1, f"expected one mapped HIP runtime, found {sorted(paths)}"
        _HIP = C.CDLL(paths.pop())
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipMemcpy.restype = C.c_int
    return _HIP


def device_views(eng, agent: int = 0):
    """(cost pointer, flags pointer, planes pointer or None, leading dimension) of an agent (fx_device_views)"""
    from frenetix_motion_planner_amd._lib import check, lib
    cost, flags, planes, ld = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
    check(lib().fx_device_views(eng._ctx, int(agent), C.byref(cost), C.byref(flags), C.byref(planes), C.byref(ld)))
    return cost.value, flags.value, planes.value, ld.value


def write_cost_flags(eng, agent, cost, flags):
    """Overwrite the first C entries of an agent's device cost and flag planes after a finished step (C = the agent's
    candidates).  `eng.costs(agent)` afterwards returns these arrays bit for bit."""
    n = eng._inputs[agent].n_candidates
    cost = np.ascontiguousarray(cost, dtype=np.float64)
    flags = np.ascontiguousarray(flags, dtype=np.uint32)
    assert cost.shape == (n,) and flags.shape == (n,), (cost.shape, flags.shape, n)
    d_cost, d_flags, _, ld = device_views(eng, agent)
    assert d_cost and d_flags and ld >= n, (d_cost, d_flags, ld, n)
    hip = _hip_runtime()
    H2D = 1   # hipMemcpyHostToDevice
    # (synchronous copies from pageable memory: complete on return, in front of whatever the engine enqueues next)
    rc = hip.hipMemcpy(C.c_void_p(d_cost), C.c_void_p(cost.ctypes.data), C.c_size_t(8 * n), H2D)
    assert rc == 0, f"hipMemcpy (cost plane) failed: {rc}"
    rc = hip.hipMemcpy(C.c_void_p(d_flags), C.c_void_p(flags.ctypes.data), C.c_size_t(4 * n), H2D)
    assert rc == 0, f"hipMemcpy (flag plane) failed: {rc}"


def bits(x):
    """the 64 bits of every double of x (of a scalar: a 0-d array, comparable and hashable through int())"""
    a = np.asarray(x, dtype=np.float64)
    return (np.ascontiguousarray(a) if a.ndim else a).view(np.uint64)


# ---- the references ----
def eligible(cost, flags):
    """selectable, neither colliding nor off the road, cost not NaN"""
    return ((flags & SEL) != 0) & ((flags & (COL | BND)) == 0) & ~np.isnan(cost)


def lex_order(cost, flags, g_base: int = 0):
    """global indices and costs of the eligible candidates in (cost, index) order"""
    el = np.nonzero(eligible(cost, flags))[0]
    order = el[np.lexsort((el, cost[el]))]
    return order + g_base, cost[order]


def expected_topk(cost, flags, k: int, g_base: int = 0):
    """(indices, costs) of topk(k): the first k of the order, padded with -1 / +inf"""
    idx, c = lex_order(cost, flags, g_base)
    n = min(k, len(idx))
    return (np.concatenate([idx[:n], np.full(k - n, -1, np.int64)]).astype(np.int64),
            np.concatenate([c[:n], np.full(k - n, np.inf)]))


def expected_selection(cost, flags):
    """(winner, its cost, collision count) of a step from its own cost / flag planes: the winner is the lexsort minimum of
    the eligible candidates; the count is the SELECTABLE & COLLISION candidates ordered before it -- all of them without a
    winner (csrc/fx_select.h, head comment)."""
    idx, c = lex_order(cost, flags)
    colliding = np.nonzero(((flags & SEL) != 0) & ((flags & COL) != 0))[0]
    if len(idx) == 0:
        return -1, None, len(colliding), colliding
    w, wc = int(idx[0]), float(c[0])
    cc = cost[colliding]
    before = (cc < wc) | ((cc == wc) & (colliding < w))
    return w, wc, int(before.sum()), colliding[before]


# ---- the planes of tests/test_topk_planes.py (each a function of the candidate count; seeded where random) ----
def _rng(name: str, n: int):
    return np.random.default_rng([20250917, n, sum(name.encode())])


def lane_of_one_slice(n: int, lane: int = 5):
    """candidates lo + lane + 64 u of the largest slice-stage slice in the middle of the agent: what ONE lane of the one-wave
    slice kernel holds in its register slots u = 0, 1, ... (at most 64 of them)"""
    per = -(-n // TOPK_SLICES)
    n_slices = -(-n // per)
    lo, hi = topk_slice_bounds(n, min(37, n_slices - 1) if n_slices > 1 else 0)
    if hi - lo <= lane:
        lane = 0
    return np.arange(lo + lane, hi, 64)[:64]


SPECIAL = np.array([-np.inf, np.inf, -0.0, 0.0, 5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308,
                    np.finfo(np.float64).max, -np.finfo(np.float64).max, 1.0, -1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)])


def _nan_payloads(rng, n):
    """NaNs of both signs, quiet and signalling, with random payloads"""
    b = rng.integers(1, 1 << 51, size=n, dtype=np.uint64) | np.uint64(0x7FF0000000000000)
    b |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)
    b |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(51)
    return b.view(np.float64)


def plane(name: str, n: int):
    """(cost, flags) of the named plane for an agent of n candidates"""
    rng = _rng(name, n)
    cost = np.zeros(n)
    flags = np.full(n, SEL, np.uint32)
    ids = np.arange(n)
    if name == "all_equal":                       # pure index order
        cost[:] = 3.25
    elif name == "three_values":                  # ties across lanes and slices
        cost = rng.choice(np.array([-1.5, 0.25, 7.0]), size=n)
    elif name == "decreasing":                    # the winner is the last candidate
        cost = (n - ids).astype(np.float64) * 0.5
    elif name in ("one_lane", "one_lane_equal"):  # the best all sit in one lane of one slice: retire and rescan in every group
        cost = rng.uniform(1.0, 2.0, size=n)
        at = lane_of_one_slice(n)
        cost[at] = -2.0 if name == "one_lane_equal" else -1.0 - rng.permutation(len(at)) / 64.0
    elif name in ("mixed_spread", "mixed_cluster", "mixed_dense"):
        # every kind of double.  Eligible NaNs fill what the named values leave: about 60 named values, so that a top-64 walks
        # through ALL of them, the zeros of both signs and +inf included (spread: over the whole agent -- they meet in the merge;
        # cluster: within two neighbouring slices -- they meet in one wave); dense: named values everywhere, top-k = the -inf ties
        cost = _nan_payloads(rng, n)
        if name == "mixed_dense":
            at = ids
        elif name == "mixed_spread" or n <= 128:
            at = ids[rng.uniform(size=n) < min(1.0, 60.0 / n)]
        else:
            lo, _ = topk_slice_bounds(n, 11)
            _, hi = topk_slice_bounds(n, 12)
            at = rng.choice(np.arange(lo, hi), size=min(60, hi - lo), replace=False)
        cost[at] = rng.choice(SPECIAL, size=len(at))
        if name == "mixed_cluster" and len(at) >= 2:   # a +0.0 in front of a -0.0: equal in the order, the index decides
            a, b = np.sort(at)[:2]
            cost[a], cost[b] = 0.0, -0.0
    elif name == "nothing_eligible":
        cost = rng.normal(size=n)
        flags = rng.choice(np.array([0, SEL | COL, SEL | BND, SEL | COL | BND, COL, _abi.FX_FLAG_VALID | _abi.FX_FLAG_FEASIBLE], np.uint32), size=n)
        nan = rng.uniform(size=n) < 0.3               # (and eligible by the flags, NaN by the cost)
        flags[nan] = SEL
        cost[nan] = np.nan
    elif name == "last_only":                     # one eligible candidate, which is the last
        cost = rng.normal(size=n)
        flags[:] = SEL | COL
        flags[-1] = SEL | _abi.FX_FLAG_VALID
    elif name == "fewer_than_k":                  # min(n, 20) eligible, scattered
        cost = rng.choice(np.array([1.0, 2.0]), size=n)
        flags[:] = 0
        flags[rng.choice(ids, size=min(n, 20), replace=False)] = SEL | _abi.FX_FLAG_COSTED
    elif name == "one_slice":                     # everything eligible inside one slice: 63 of the merge's 64 lists are empty
        cost = rng.choice(np.array([4.0, 5.0, 6.0]), size=n)
        flags[:] = SEL | BND
        lo, hi = topk_slice_bounds(n, min(41, -(-n // -(-n // TOPK_SLICES)) - 1))
        flags[lo:hi] = SEL
    elif name == "flag_reasons":                  # each flag reason excludes a candidate that would otherwise win
        cost = rng.uniform(1.0, 2.0, size=n)
        for j, f in enumerate((_abi.FX_FLAG_VALID | _abi.FX_FLAG_COSTED, SEL | COL, SEL | BND)):   # (not selectable; colliding; off the road)
            g = (j * (n // 3) + n // 7) % n
            cost[g], flags[g] = -5.0 + j, f
        if n > 3:
            g = (n // 2 + 1) % n
            if flags[g] == SEL:
                cost[g] = 0.5                     # the winner that is left
    elif name == "only_inf":                      # only +inf costs are eligible: infinite is still a candidate
        cost = rng.uniform(-2.0, 2.0, size=n)
        flags[:] = SEL | COL
        at = ids[rng.uniform(size=n) < max(0.3, min(1.0, 40.0 / n))] if n > 1 else ids
        cost[at], flags[at] = np.inf, SEL
    else:
        raise KeyError(name)
    return np.ascontiguousarray(cost, dtype=np.float64), np.ascontiguousarray(flags, dtype=np.uint32)


PLANES = ("all_equal", "three_values", "decreasing", "one_lane", "one_lane_equal", "mixed_spread", "mixed_cluster", "mixed_dense",
          "nothing_eligible", "last_only", "fewer_than_k", "one_slice", "flag_reasons", "only_inf")
