"""The four top-k kernels (csrc/fx_topk_kernel.h; launcher: csrc/fx_kernels.hip) on planes written by the test, at the sizes where fx_launch_topk changes kernels.

Slice stage: fx_topk_slice_wave_kernel while ceil(C / 64) <= 64 x 32, i.e. up to 131 072 candidates (every register slot of
every lane full there), fx_topk_slice_kernel from 131 073 on.  Merge stage: fx_topk_merge_wave_kernel up to k = 32,
fx_topk_merge_kernel above.  In a batch the largest agent decides.  `test_switch_sizes_follow_the_source` (no GPU) derives these
sizes, and those of tests/test_select_sizes.py, from the constants in csrc/ and fails when they move.

Reference: NumPy on the written planes (tests/device_planes.py): eligible = SELECTABLE, neither COLLISION nor BOUNDARY, cost not
NaN; order = np.lexsort((global index, cost)); expected = its first k, padded with index -1 and cost +inf.  Indices are compared
for equality, costs BIT for bit -- except that a zero may come back with the other sign: the one-wave kernels add 0.0 to every cost
they load (their integer sort keys know no negative zero), the general kernels hand a -0.0 through as it is.  -0.0 == +0.0 in the
order (the index decides between them), so `same_costs` compares zeros with == and everything else by its bits;
`test_zero_sign_tells_which_kernels_ran` then pins the sign itself to the kernels the launcher must have taken.

The scene behind an engine only has to give the candidate count: a select-only step (no bundle, no cost map), no obstacles, a
1.5 s horizon, the first C rows of a 200 000-row sampling matrix."""
import os

import numpy as np
import pytest

from frenetix_motion_planner_amd import synthetic
from tests import device_planes as dp

KS = dp.TOPK_KS
CSRC = os.path.join(os.path.dirname(os.path.abspath(synthetic.__file__)), "csrc")
N_ROWS = 200_000
_BASE = {}


def count_scene(C: int, *, shard=None):
    """select-only PlanInputs of exactly C candidates (or the shard [begin, begin + count) of the whole matrix)"""
    import copy
    if "inp" not in _BASE:
        _BASE["inp"] = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(5, 200, 199), n_obstacles=0, horizon=1.5, n_pred=15, as_matrix=True,
                                             write_bundle=False, write_costmap=False)
        assert _BASE["inp"].n_candidates == N_ROWS
    inp = copy.copy(_BASE["inp"])
    if shard is None:
        inp.sampling_matrix = np.ascontiguousarray(inp.sampling_matrix[:C])
    inp.shard = shard
    assert inp.n_candidates == C and not inp.write_bundle and inp.mode == 0
    return inp


def same_costs(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool(np.all((dp.bits(got) == dp.bits(want)) | ((got == 0.0) & (want == 0.0))))


def hold_topk(e, planes, ks=KS, g_bases=None, what=""):
    """topk(k) of the engine's agents against the reference on `planes` = [(cost, flags) per agent]; returns {k: (cost, index)}"""
    orders = [dp.lex_order(c, f, 0 if g_bases is None else g_bases[a]) for a, (c, f) in enumerate(planes)]
    rows = {}
    for k in ks:
        c, i = e.topk(k)
        assert c.shape == i.shape == (len(planes), k)
        for a, (idx, cc) in enumerate(orders):
            n = min(k, len(idx))
            want_i = np.concatenate([idx[:n], np.full(k - n, -1, np.int64)])
            want_c = np.concatenate([cc[:n], np.full(k - n, np.inf)])
            assert np.array_equal(i[a], want_i), (what, k, a, i[a][:8], want_i[:8])
            assert same_costs(c[a], want_c), (what, k, a, c[a][:8], want_c[:8])
        rows[k] = (c, i)
    return rows


@pytest.fixture(scope="module")
def engines():
    """one engine per candidate count, each behind one finished select-only step"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    made = {}

    def get(C):
        if C not in made:
            inp = count_scene(C)
            e = FrenetEngine(max_candidates=C + 64, max_steps=inp.N)
            e.plan_step(inp)
            made[C] = e
        return made[C]

    yield get
    for e in made.values():
        e.close()


# ---- without a GPU: the sizes, the reference, the planes ----
def test_switch_sizes_follow_the_source():
    """The sizes both GPU modules are parametrised on, derived from the constants in csrc/: a change there fails here instead of
    leaving the GPU tests beside the switches."""
    k = dp.source_constants(CSRC)
    assert k["topk_slices"] == dp.TOPK_SLICES == 64 and k["topk_r"] == 32
    wave_max = k["topk_slices"] * 64 * k["topk_r"]          # per = ceil(C / slices) <= 64 * R
    assert wave_max == dp.TOPK_WAVE_MAX_C == 131_072
    assert {wave_max, wave_max + 1} <= set(dp.TOPK_SIZES)
    assert -(-wave_max // k["topk_slices"]) == 64 * k["topk_r"] and -(-(wave_max + 1) // k["topk_slices"]) == 64 * k["topk_r"] + 1
    k_max = 64 * k["topk_r"] // k["topk_slices"]            # slices * k <= 64 * R
    assert k_max == dp.TOPK_WAVE_MAX_K == 32 and {k_max - 1, k_max, k_max + 1, 64, 1} == set(dp.TOPK_KS)
    # the remaining top-k sizes: one wave's lanes (63 / 64 / 65) and one candidate per lane of every slice (4 096 / 4 097)
    assert {1, 63, 64, 65, 64 * k["topk_slices"], 64 * k["topk_slices"] + 1} <= set(dp.TOPK_SIZES)
    assert max(dp.TOPK_SIZES) > wave_max + 1 and max(dp.TOPK_SIZES) % k["topk_slices"] != 0 and max(dp.TOPK_SIZES) <= N_ROWS
    # selection: slices, candidates per slice, pre-loaded pairs
    assert k["select_slices_min"] == dp.SELECT_SLICES_MIN == 32 and k["select_slices_max"] == 512
    assert k["per_slice"] == dp.SELECT_PER_SLICE == 4_096 and k["batch_workgroups"] == dp.SELECT_BATCH_WORKGROUPS == 2_048
    assert k["preload_pairs"] * 256 == dp.SELECT_PRELOAD == 2_048 and k["second_loop_start"] == (k["preload_pairs"], 256)
    second_loop_above = k["select_slices_min"] * dp.SELECT_PRELOAD
    doubles_above = k["select_slices_min"] * k["per_slice"]
    assert dp.SELECT_SIZES == (second_loop_above, second_loop_above + 1, doubles_above, doubles_above + 1, 2 * doubles_above + 1)
    assert [dp.select_slices(c) for c in dp.SELECT_SIZES] == [32, 32, 32, 64, 128]
    assert [-(-c // dp.select_slices(c)) for c in dp.SELECT_SIZES] == [2_048, 2_049, 4_096, 2_049, 2_049]
    assert dp.select_slices(1_000_000) == 256 and dp.select_slices(10**7) == 512
    assert dp.select_slices(doubles_above + 1, 33) == 32 and dp.select_slices(doubles_above + 1, 32) == 64


def test_reference_is_pythons_stable_sort():
    """expected_topk / expected_selection against sorted() on small planes: Python's stable sort IS the rule"""
    for name in dp.PLANES:
        for n in (1, 63, 65, 700):
            cost, flags = dp.plane(name, n)
            el = [g for g in range(n) if (flags[g] & dp.SEL) and not (flags[g] & (dp.COL | dp.BND)) and cost[g] == cost[g]]
            order = sorted(el, key=lambda g: cost[g])
            for k in (1, 33, 64):
                i, c = dp.expected_topk(cost, flags, k, g_base=1000)
                assert list(i) == [g + 1000 for g in order[:k]] + [-1] * (k - len(order[:k]))
                assert same_costs(c, [cost[g] for g in order[:k]] + [np.inf] * (k - len(order[:k]))) and \
                    np.array_equal(dp.bits(c[:len(order[:k])]), dp.bits(cost[order[:k]]))
            flags = flags.copy()
            flags[::3] |= dp.COL                                  # (a third collides)
            el = [g for g in range(n) if (flags[g] & dp.SEL) and not (flags[g] & (dp.COL | dp.BND)) and cost[g] == cost[g]]
            free = set(el)
            walk = sorted((g for g in range(n) if (flags[g] & dp.SEL) and ((flags[g] & dp.COL) or g in free)), key=lambda g: cost[g])
            # the reference's walk: cost order, colliding candidates counted until the first one that is free
            w, wc, count, _ = dp.expected_selection(cost, flags)
            if el:
                first = min(el, key=lambda g: (cost[g], g))
                assert w == first
                seen = [g for g in range(n) if (flags[g] & dp.SEL) and (flags[g] & dp.COL) and (cost[g] < cost[w] or (cost[g] == cost[w] and g < w))]
                assert count == len(seen)
                if not any(cost[g] != cost[g] for g in walk):
                    assert count == sum(1 for g in walk[:walk.index(w)] if flags[g] & dp.COL)
            else:
                assert w == -1 and count == sum(1 for g in range(n) if (flags[g] & dp.SEL) and (flags[g] & dp.COL))


def test_planes_are_what_their_names_say():
    from frenetix_motion_planner_amd import _abi
    for n in dp.TOPK_SIZES:
        for name in dp.PLANES:
            cost, flags = dp.plane(name, n)
            assert cost.shape == flags.shape == (n,) and cost.dtype == np.float64 and flags.dtype == np.uint32
            c2, f2 = dp.plane(name, n)
            assert np.array_equal(dp.bits(cost), dp.bits(c2)) and np.array_equal(flags, f2)      # seeded
        per = -(-n // 64)
        idx, c = dp.lex_order(*dp.plane("one_lane", n))
        at = dp.lane_of_one_slice(n)
        assert set(idx[:len(at)]) == set(at) and np.all((at - at[0]) % 64 == 0) and len(np.unique(at // per)) == 1
        assert len(at) == min(64, -(-(per - (at[0] - at[0] // per * per)) // 64))       # as many as the lane holds
        if n == dp.TOPK_WAVE_MAX_C:
            slots = (at - at[0]) // 64
            assert len(at) == 32 and set(slots // 8) == {0, 1, 2, 3}          # every group of eight register slots, full
            order = (idx[:32] - at[0]) // 64 // 8
            assert np.count_nonzero(np.diff(order)) > 8                       # and the order jumps between the groups
        idx, c = dp.lex_order(*dp.plane("one_lane_equal", n))
        assert np.array_equal(idx[:len(at)], at) and len(np.unique(c[:len(at)])) == 1
        assert len(dp.lex_order(*dp.plane("nothing_eligible", n))[0]) == 0
        assert list(dp.lex_order(*dp.plane("last_only", n))[0]) == [n - 1]
        assert len(dp.lex_order(*dp.plane("fewer_than_k", n))[0]) == min(n, 20)
        idx, _ = dp.lex_order(*dp.plane("decreasing", n))
        assert idx[0] == n - 1 and np.array_equal(idx[:64], np.arange(n - 1, -1, -1)[:64])
        idx, _ = dp.lex_order(*dp.plane("one_slice", n))
        assert len(idx) > 0 and len(np.unique(idx // per)) == 1
        idx, c = dp.lex_order(*dp.plane("only_inf", n))
        assert len(idx) > 0 and np.all(c == np.inf)
        if n >= 63:
            cost, flags = dp.plane("flag_reasons", n)
            losers = np.argsort(cost)[:3]                                      # the three cheapest are the three excluded
            assert sorted(int(f) for f in flags[losers]) == sorted([_abi.FX_FLAG_VALID | _abi.FX_FLAG_COSTED, dp.SEL | dp.COL, dp.SEL | dp.BND])
            assert dp.lex_order(cost, flags)[0][0] not in losers
        if n >= 4_096:
            for name in ("mixed_spread", "mixed_cluster"):
                cost, flags = dp.plane(name, n)
                idx, c = dp.lex_order(cost, flags)
                assert 30 <= len(idx) <= 100 and np.isnan(cost).sum() >= n - 100 and np.all(flags == dp.SEL)
                got = set(dp.bits(c).tolist())
                assert len(got) >= 12 and {int(dp.bits(x)) for x in (-0.0, 0.0, np.inf, -np.inf)} <= got
            idx, _ = dp.lex_order(*dp.plane("mixed_cluster", n))
            assert len(np.unique(idx // per)) <= 2
            z = [g for g in idx if cost[g] == 0.0]
            # a +0.0 in front of a -0.0 in one slice: keys that knew a negative zero would order them the other way
            assert any(not np.signbit(cost[a]) and np.signbit(cost[b]) and a // per == b // per for a in z for b in z if a < b), n


def test_helper_imports_without_a_gpu():
    """the module both GPU modules build on loads, and answers, on a host without a device"""
    assert callable(dp.write_cost_flags) and callable(dp.device_views)
    cost, flags = dp.plane("mixed_dense", 65)
    assert dp.eligible(cost, flags).sum() == np.count_nonzero(~np.isnan(cost)) > 0


# ---- on the GPU ----
@pytest.mark.gpu
def test_written_planes_read_back_bit_for_bit(engines):
    """write_cost_flags: costs() afterwards returns what was written -- NaN payloads, the sign of zero, every flag bit"""
    for C in (65, 4_097):
        e = engines(C)
        rng = np.random.default_rng(C)
        cost, _ = dp.plane("mixed_dense", C)
        cost[::5] = dp.plane("mixed_spread", C)[0][::5]               # (NaNs with payloads)
        flags = rng.integers(0, 1 << 32, size=C, dtype=np.uint64).astype(np.uint32)
        assert np.isnan(cost).any() and np.any(dp.bits(cost) == dp.bits(-0.0)) and np.any(dp.bits(cost) == dp.bits(0.0))
        dp.write_cost_flags(e, 0, cost, flags)
        c2, f2 = e.costs()
        assert np.array_equal(dp.bits(c2), dp.bits(cost)) and np.array_equal(f2, flags)
        d_cost, d_flags, planes, ld = dp.device_views(e)
        assert d_cost and d_flags and planes is None and ld >= C       # (select-only: no bundle planes)


@pytest.mark.gpu
@pytest.mark.parametrize("name", dp.PLANES)
@pytest.mark.parametrize("C", dp.TOPK_SIZES)
def test_topk_on_written_planes(C, name, engines):
    e = engines(C)
    cost, flags = dp.plane(name, C)
    dp.write_cost_flags(e, 0, cost, flags)
    hold_topk(e, [(cost, flags)], what=(C, name))


@pytest.mark.gpu
@pytest.mark.parametrize("C", (dp.TOPK_WAVE_MAX_C, dp.TOPK_WAVE_MAX_C + 1))
def test_zero_sign_tells_which_kernels_ran(C, engines):
    """Every cost -0.0.  A one-wave kernel on the way (slice stage up to 131 072 candidates, merge stage up to k = 32) returns
    +0.0; only the two general kernels together hand the written sign through -- so the sign shows on which side of BOTH
    conditions of fx_launch_topk a call went."""
    e = engines(C)
    cost, flags = np.full(C, -0.0), np.full(C, dp.SEL, np.uint32)
    dp.write_cost_flags(e, 0, cost, flags)
    for k in (dp.TOPK_WAVE_MAX_K, dp.TOPK_WAVE_MAX_K + 1):
        c, i = e.topk(k)
        assert np.array_equal(i[0], np.arange(k))
        general = C > dp.TOPK_WAVE_MAX_C and k > dp.TOPK_WAVE_MAX_K
        assert np.all(c[0] == 0.0) and np.all(np.signbit(c[0]) == general), (C, k, c[0])


@pytest.mark.gpu
def test_batch_follows_its_largest_agent(engines):
    """Agents of 1, 63 and 131 073 candidates in one batch: the general slice kernel for all three (the small agents leave 63 and
    one of its 64 slices empty); each agent's rows equal the rows of the agent alone."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    sizes = (1, 63, dp.TOPK_WAVE_MAX_C + 1)
    inps = [count_scene(C) for C in sizes]
    with FrenetEngine(max_candidates=sum(sizes) + 64 * len(sizes), max_steps=inps[0].N, max_agents=len(sizes)) as e:
        e.plan_batch(inps)
        for names in (("mixed_dense", "three_values", "three_values"), ("only_inf", "mixed_dense", "mixed_cluster"),
                      ("all_equal", "all_equal", "one_lane_equal"), ("nothing_eligible", "decreasing", "last_only")):
            planes = [dp.plane(nm, C) for nm, C in zip(names, sizes)]
            for a, (c, f) in enumerate(planes):
                dp.write_cost_flags(e, a, c, f)
            rows = hold_topk(e, planes, what=names)
            for a, C in enumerate(sizes):
                alone = engines(C)
                dp.write_cost_flags(alone, 0, *planes[a])
                for k in KS:
                    c1, i1 = alone.topk(k)
                    assert np.array_equal(i1[0], rows[k][1][a]) and same_costs(c1[0], rows[k][0][a]), (names, a, k)


@pytest.mark.gpu
@pytest.mark.parametrize("begin,count", [(60_000, dp.TOPK_WAVE_MAX_C + 1), (68_927, dp.TOPK_WAVE_MAX_C), (199_937, 63)])
def test_sharded_agent_answers_global_indices(begin, count):
    """PlanInputs.shard with a non-zero begin: the planes hold the shard's candidates, the indices that come back are global"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = count_scene(count, shard=(begin, count))
    assert inp.shard_begin == begin and inp.n_candidates_global == N_ROWS
    with FrenetEngine(max_candidates=N_ROWS + 64, max_steps=inp.N) as e:      # (the whole matrix is uploaded, the shard evaluated)
        e.plan_step(inp)
        for name in ("three_values", "one_lane_equal", "mixed_cluster", "fewer_than_k"):
            cost, flags = dp.plane(name, count)
            dp.write_cost_flags(e, 0, cost, flags)
            rows = hold_topk(e, [(cost, flags)], g_bases=[begin], what=(begin, count, name))
        assert rows[64][1][0].max() >= begin


@pytest.mark.gpu
def test_k_outside_one_to_sixty_four_is_refused(engines):
    e = engines(65)
    for k in (0, 65):
        with pytest.raises(ValueError, match="outside"):
            e.topk(k)
    c, i = e.topk(64)
    assert c.shape == (1, 64)
