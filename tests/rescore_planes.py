"""Raw cost rows and flag planes written by a test for the re-score kernels (csrc/fx_rescore_kernel.h), and the
plain NumPy statement of what they must answer.

`fx_rescore_agent` reads an agent's raw cost rows [n_cost][ld] and its flag plane afresh on every call.  `write_rows` overwrites both
on the device after a finished step -- the rows through `fx_device_costmap_view`, the flags through `fx_device_views`, host-to-device
copies through the HIP runtime the library has already loaded (the route of tests/device_planes.py) -- so a test can show the kernels
any plane: ties by construction, NaN, infinities, every flag reason.

The reference is the sequence of multiplications and additions of fx_cost_sum.h, element-wise in NumPy: every operation is one IEEE
binary64 operation on both sides -- the library is built with -ffp-contract=off (csrc/Makefile; `contraction_is_off` checks it),
and NumPy fuses nothing -- so totals, winner and cost are compared exactly.  Importable without a GPU."""
import ctypes as C
import os
import re

import numpy as np

from frenetix_motion_planner_amd import _abi, synthetic
from frenetix_motion_planner_amd.problem import DEFAULT_COST_WEIGHTS
from tests import device_planes as dp

CSRC = os.path.join(os.path.dirname(os.path.abspath(synthetic.__file__)), "csrc")
SEL, COL, BND, COSTED = _abi.FX_FLAG_SELECTABLE, _abi.FX_FLAG_COLLISION, _abi.FX_FLAG_BOUNDARY, _abi.FX_FLAG_COSTED
OK = SEL | COSTED | _abi.FX_FLAG_VALID | _abi.FX_FLAG_FEASIBLE
LANE, VECTOR = 1, 2

# ---- the sizes at which the pass changes its code path (tests/test_rescore_plan.py derives them from csrc/fx_rescore_plan.h) ----
VECTOR_MIN = 64                       # vectors from which a wave of them is full: the vector regime
TILE = 256                            # candidates of a lane-regime workgroup
SIZES = (1, 63, 64, 65, 257, 4_097)   # one lane; a wave -1 / full / +1; a tile + 1; 17 tiles, the last of ONE candidate
N_VECS = tuple(sorted({1, 63, 64, 65, VECTOR_MIN - 1, VECTOR_MIN, VECTOR_MIN + 1}))


def source_constants() -> dict:
    """the #defines of csrc/fx_rescore_plan.h the sizes above follow from, and the rule's condition as written"""
    hdr = open(os.path.join(CSRC, "fx_rescore_plan.h")).read()

    def one(pattern):
        m = re.findall(pattern, hdr)
        assert len(m) == 1, (pattern, m)
        return m[0]

    out = {name.lower(): int(one(rf"#define FX_RESCORE_{name} (\d+)\b")) for name in
           ("LANE", "VECTOR", "TILE", "CHUNK_MAX", "VECTOR_MIN", "WORKGROUPS", "WAVES", "SLICE_MIN", "MAX_VECTORS")}
    assert one(r"n_vec (>=?) FX_RESCORE_VECTOR_MIN \? FX_RESCORE_VECTOR : FX_RESCORE_LANE") == ">="
    return out


def contraction_is_off() -> bool:
    """the library's device and host code is compiled without multiply-add contraction, so the reference must not fuse either"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    return "-ffp-contract=off" in flags and "-ffp-contract=fast" not in mk and "-ffast-math" not in flags


# ---- the scene behind an engine: it only has to give the candidate count and a cost list with a prediction term ----
_BASE = {}


def count_scene(n: int):
    """PlanInputs of exactly n candidates that store bundle and cost map: the first n rows of a 5 x 30 x 30 sampling matrix, no
    obstacles, the default five cost terms (the prediction among them)"""
    import copy
    if "inp" not in _BASE:
        _BASE["inp"] = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(5, 30, 30), n_obstacles=0, horizon=1.5, n_pred=15, as_matrix=True,
                                             cost_weights=dict(DEFAULT_COST_WEIGHTS))
        assert _BASE["inp"].n_candidates >= max(SIZES)
    inp = copy.copy(_BASE["inp"])
    inp.sampling_matrix = np.ascontiguousarray(inp.sampling_matrix[:n])
    assert inp.n_candidates == n and inp.write_bundle and (inp.mode & _abi.FX_MODE_WRITE_COSTMAP) and "prediction" in inp.cost_names
    return inp


# ---- writing the planes ----
def costmap_view(eng, agent: int = 0):
    """(device pointer of the raw cost rows, leading dimension, n_cost) of an agent (fx_device_costmap_view)"""
    from frenetix_motion_planner_amd._lib import check, lib
    p, ld, n_cost = C.c_void_p(), C.c_int64(0), C.c_int32(0)
    check(lib().fx_device_costmap_view(eng._ctx, int(agent), C.byref(p), C.byref(ld), C.byref(n_cost)))
    return p.value, ld.value, n_cost.value


def write_rows(eng, agent, raw, flags):
    """Overwrite an agent's raw cost rows (raw [n_cost][n]) and its flag plane (flags [n]) on the device after a finished step.
    `eng.costmap(agent)` afterwards returns raw.T bit for bit."""
    n = eng._inputs[agent].n_candidates
    raw = np.ascontiguousarray(raw, dtype=np.float64)
    flags = np.ascontiguousarray(flags, dtype=np.uint32)
    d_rows, ld, n_cost = costmap_view(eng, agent)
    assert raw.shape == (n_cost, n) and flags.shape == (n,) and d_rows and ld >= n, (raw.shape, flags.shape, n_cost, n, ld)
    _, d_flags, _, ld2 = dp.device_views(eng, agent)
    assert d_flags and ld2 == ld
    hip = dp._hip_runtime()
    H2D = 1   # hipMemcpyHostToDevice
    for m in range(n_cost):   # (synchronous copies from pageable memory: complete on return; row m starts at m * ld doubles)
        rc = hip.hipMemcpy(C.c_void_p(d_rows + 8 * m * ld), C.c_void_p(raw[m].ctypes.data), C.c_size_t(8 * n), H2D)
        assert rc == 0, f"hipMemcpy (cost row {m}) failed: {rc}"
    rc = hip.hipMemcpy(C.c_void_p(d_flags), C.c_void_p(flags.ctypes.data), C.c_size_t(4 * n), H2D)
    assert rc == 0, f"hipMemcpy (flag plane) failed: {rc}"


# ---- the reference ----
def totals_of(raw, flags, w, n_pred: int, deferred: bool):
    """total [n] of one weight vector w [n_cost] over raw [n_cost][n]: fx_cost_sum.h, operation by operation; NaN without COSTED"""
    n_cost, n = raw.shape
    defer = bool(deferred) and n_pred >= 0
    s, tail = np.full(n, -0.0), np.zeros(n)
    with np.errstate(all="ignore"):
        for m in range(n_cost):
            t = np.float64(w[m]) * raw[m]
            if defer and m > n_pred:
                tail = tail + t
            else:
                s = s + t
        if defer and n_pred + 1 < n_cost:
            s = s + tail
        total = 0.0 + s
    return np.where((flags & COSTED) != 0, total, np.nan)


def winner_of(total, flags):
    """(index, cost) of the lexicographic (total, index) minimum over the eligible candidates; (-1, +inf) without one"""
    el = np.nonzero(dp.eligible(total, flags))[0]
    if len(el) == 0:
        return -1, np.inf
    g = int(el[np.lexsort((el, total[el]))][0])
    return g, float(total[g])


def expected(raw, flags, W, n_pred: int, deferred: bool):
    """(winner [W], cost [W], totals [W][n]) of the weight vectors W [n_vec][n_cost]"""
    tot = np.stack([totals_of(raw, flags, w, n_pred, deferred) for w in W])
    win = [winner_of(t, flags) for t in tot]
    return np.array([g for g, _ in win], np.int64), np.array([c for _, c in win]), tot


def same_nan_or_bits(got, want):
    """bit for bit, any NaN standing for any NaN (the kernels write the quiet NaN, NumPy's np.nan is the same one, but a NaN that came
    out of inf - inf carries the sign the hardware gave it)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(np.all((dp.bits(got) == dp.bits(want)) | (np.isnan(got) & np.isnan(want))))


# ---- weight vectors and planes (functions of the sizes; seeded where random) ----
def _rng(name: str, *k):
    return np.random.default_rng([20251021, sum(name.encode()), *k])


def weight_vectors(n_vec: int, n_cost: int):
    """[n_vec][n_cost]: finite, not zero, both signs, magnitudes from 1e-3 to 1e3; vector 0 is all ones, vector 1 all ones but a
    -1 in front: what the tie planes below are built on"""
    rng = _rng("weights", n_vec, n_cost)
    W = rng.choice(np.array([-1.0, 1.0]), size=(n_vec, n_cost), p=[0.25, 0.75]) * 10.0 ** rng.uniform(-3, 3, size=(n_vec, n_cost))
    W[0] = 1.0
    if n_vec > 1:
        W[1] = 1.0
        W[1, 0] = -1.0
    assert np.all(np.isfinite(W)) and np.all(W != 0.0)
    return np.ascontiguousarray(W)


PLANES = ("all_equal", "ties_under_some", "non_finite", "nothing_eligible", "flag_reasons", "last_wins")


def plane(name: str, n: int, n_cost: int):
    """(raw [n_cost][n], flags [n]) of the named plane"""
    rng = _rng(name, n, n_cost)
    raw = rng.uniform(0.5, 2.0, size=(n_cost, n))
    flags = np.full(n, OK, np.uint32)
    if name == "all_equal":                   # every candidate the same rows: the lowest eligible index wins under every vector
        raw[:] = raw[:, :1]
        flags[: n // 3] = SEL | COL | COSTED   # (and that is not candidate 0 from n = 3 on)
    elif name == "ties_under_some":           # two candidates that tie under the all-ones vector 0 and not under vector 1
        raw[:] = np.floor(raw * 8.0) / 8.0 + 3.0      # (multiples of 1/8: the sums below are exact)
        a, b = (n // 3, n - 1) if n > 1 else (0, 0)
        raw[:, a] = 1.0
        raw[:, b] = 1.0
        if n > 1 and n_cost > 1:
            raw[0, a], raw[1, a] = 0.5, 1.5           # the same sum of rows, another first row
    elif name == "non_finite":                # NaN and +-inf raw costs: NaN totals are skipped, infinite ones take part
        raw[rng.integers(0, n_cost, size=n), np.arange(n)] = rng.choice(np.array([np.nan, np.inf, -np.inf, 1.0, 2.0]), size=n)
    elif name == "nothing_eligible":
        flags = rng.choice(np.array([0, COSTED, SEL | COL | COSTED, SEL | BND | COSTED, SEL | COL | BND | COSTED, SEL], np.uint32), size=n)
        raw[0, (flags == SEL)] = np.nan        # (selectable without a cost: NaN by the flag, and by the row)
    elif name == "flag_reasons":              # each flag reason excludes a candidate that would otherwise win under positive weights
        for j, f in enumerate((COSTED | _abi.FX_FLAG_VALID, SEL | COL | COSTED, SEL | BND | COSTED)):   # not selectable; colliding; off the road
            g = (j * (n // 3) + n // 7) % n
            raw[:, g], flags[g] = 0.001 * (j + 1), f
    elif name == "last_wins":                 # the winner under positive weights is the last candidate
        raw[:, -1] = 0.01
    else:
        raise KeyError(name)
    return np.ascontiguousarray(raw), np.ascontiguousarray(flags)
