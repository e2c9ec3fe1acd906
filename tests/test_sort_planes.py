"""The device sort (csrc/fx_sort_kernel.h) on planes written by the test, at the sizes where fx_launch_sort
changes its code path: fx_sort_small_kernel (one workgroup, one launch) up to 4 096 candidates, histogram / offsets / scatter per
pass over tiles of 2 048 keys above.  tests/test_sort_host.py (no GPU) derives the sizes from the #defines and holds the reference
to Python's stable sort.

Reference: tests/sort_planes.reference_order -- pool[np.argsort(cost[pool], kind="stable")].  Everything is compared exactly: the
whole order, n_pool, n_nan, and the costs and flag words of every rank BIT for bit against cost[ids], flags[ids] (the sort never
rebuilds a cost from a key: NaN payloads and the sign of zero come back as written).

The scene behind an engine only has to give the candidate count (tests/test_topk_planes.count_scene: a select-only step without
obstacles, the first C rows of a 200 000-row sampling matrix)."""
import ctypes as C

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import device_planes as dp
from tests import sort_planes as sp
from tests.test_topk_planes import N_ROWS, count_scene

pytestmark = pytest.mark.gpu
NOT_READY, INVALID = f"status {_abi.FX_ERR_NOT_READY}", f"status {_abi.FX_ERR_INVALID_ARGUMENT}"


@pytest.fixture(scope="module")
def engines():
    """one engine per candidate count, each behind one finished select-only step"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    made = {}

    def get(n):
        if n not in made:
            inp = count_scene(n)
            e = FrenetEngine(max_candidates=n + 64, max_steps=inp.N)
            e.plan_step(inp)
            made[n] = e
        return made[n]

    yield get
    for e in made.values():
        e.close()


def hold_order(e, cost, flags, require, exclude, agent=0, what=""):
    """sort the agent and hold counts, order, costs and flags of every rank, and ranges at both ends and across a tile boundary"""
    want, want_nan = sp.reference_order(cost, flags, require, exclude)
    n_pool, n_nan = e.sort_candidates(agent, require, exclude)
    assert (n_pool, n_nan) == (len(want), want_nan), (what, n_pool, n_nan, len(want), want_nan)
    ids, c, f = e.ranked(0, n_pool, agent, with_cost=True)
    assert ids.dtype == np.int64 and np.array_equal(ids, want), (what, ids[:8], want[:8], int(np.argmax(ids != want)) if n_pool else -1)
    assert np.array_equal(dp.bits(c), dp.bits(cost[want])) and np.array_equal(f, flags[want]), what
    assert len(e.ranked(n_pool, 0, agent)) == 0 and len(e.ranked(0, 0, agent)) == 0              # n == 0 is legal, at either end
    for first, n in ((0, 3), (n_pool - 3, 3), (sp.SORT_TILE - 9, 20), (n_pool // 2, 1)):
        if first >= 0 and first + n <= n_pool:
            i2, c2, f2 = e.ranked(first, n, agent, with_cost=True)
            assert np.array_equal(i2, want[first:first + n]) and np.array_equal(e.ranked(first, n, agent), i2), (what, first, n)
            assert np.array_equal(dp.bits(c2), dp.bits(cost[i2])) and np.array_equal(f2, flags[i2]), (what, first, n)
    p, n_view = e.sort_view(agent)
    assert p and n_view == n_pool
    return want, want_nan


# ---- sizes x planes x pools ----
@pytest.mark.parametrize("n", sp.SORT_SIZES)
def test_order_on_written_planes(n, engines):
    e = engines(n)
    for name in sp.ALL_PLANES:
        cost, flags = sp.any_plane(name, n)
        dp.write_cost_flags(e, 0, cost, flags)
        for require, exclude in sp.POOLS:
            want, n_nan = hold_order(e, cost, flags, require, exclude, what=(n, name, require))
            if (require, exclude) == (sp.SEL, sp.COL | sp.BND):
                # the first ranks of the survivor pool are the top-k (which skips NaN costs: the order's last n_nan ranks)
                _, idx = e.topk(64)
                k = min(64, len(want) - n_nan)
                assert np.array_equal(idx[0][:k], want[:k]) and np.all(idx[0][k:] == -1), (n, name)


def test_planes_cover_the_named_pools(engines):
    """an empty pool and a pool of one, which is the last candidate -- at a one-workgroup size and at a tiled one"""
    for n in (sp.SORT_TILE + 1, sp.SORT_SMALL_MAX + 1):
        e = engines(n)
        cost, flags = dp.plane("all_equal", n)                      # every flag word SELECTABLE alone: nothing is COSTED
        dp.write_cost_flags(e, 0, cost, flags)
        assert e.sort_candidates(0, sp.COSTED, 0) == (0, 0) and len(e.ranked(0, 0)) == 0
        with pytest.raises(ValueError, match=INVALID):
            e.ranked(0, 1)
        cost, flags = dp.plane("last_only", n)
        dp.write_cost_flags(e, 0, cost, flags)
        assert e.sort_candidates(0, sp.SEL, sp.COL | sp.BND) == (1, 0)
        ids, c, f = e.ranked(0, 1, with_cost=True)
        assert ids.tolist() == [n - 1] and dp.bits(c)[0] == dp.bits(cost)[n - 1] and f[0] == flags[n - 1]


# ---- a batch of agents ----
@pytest.mark.parametrize("largest", (sp.SORT_TILE + 1, sp.SORT_SMALL_MAX + 1))
def test_batch_follows_its_largest_agent(largest, engines):
    """Agents of 1, 63 and `largest` candidates sorted by ONE call: the largest chooses the decomposition (one workgroup per agent up
    to 4 096, tiles above -- the small agents then leave all tiles but their first empty); every agent's order equals the order of
    the agent alone."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    sizes = (1, 63, largest)
    inps = [count_scene(n) for n in sizes]
    with FrenetEngine(max_candidates=sum(sizes) + 64 * len(sizes), max_steps=inps[0].N, max_agents=len(sizes)) as e:
        e.plan_batch(inps)
        for names in (("mixed_dense", "nan_between", "signs_interleaved"), ("byte_3", "three_values", "nan_between"),
                      ("nothing_eligible", "descending", "digits_0_255")):
            planes = [sp.any_plane(nm, n) for nm, n in zip(names, sizes)]
            for a, (c, f) in enumerate(planes):
                dp.write_cost_flags(e, a, c, f)
            for require, exclude in sp.POOLS:
                n_pool, n_nan = e.sort_candidates_batch(require, exclude)
                for a, (c, f) in enumerate(planes):
                    want, want_nan = sp.reference_order(c, f, require, exclude)
                    assert (n_pool[a], n_nan[a]) == (len(want), want_nan), (names, a, require)
                    ids, cc, ff = e.ranked(0, len(want), a, with_cost=True)
                    assert np.array_equal(ids, want) and np.array_equal(dp.bits(cc), dp.bits(c[want])) and np.array_equal(ff, f[want])
                    alone = engines(sizes[a])
                    dp.write_cost_flags(alone, 0, c, f)
                    assert alone.sort_candidates(0, require, exclude) == (len(want), want_nan)
                    assert np.array_equal(alone.ranked(0, len(want)), ids), (names, a, require)
            # one agent sorted again on its own leaves the others' orders readable
            want0, _ = sp.reference_order(*planes[0], 0, 0)
            want2, _ = sp.reference_order(*planes[2], sp.SEL, 0)
            e.sort_candidates_batch(0, 0)
            assert e.sort_candidates(2, sp.SEL, 0)[0] == len(want2)
            assert np.array_equal(e.ranked(0, len(want2), 2), want2) and np.array_equal(e.ranked(0, len(want0), 0), want0)


# ---- a shard ----
@pytest.mark.parametrize("begin,count", [(60_000, sp.SORT_SMALL_MAX + 1), (199_937, 63)])
def test_sharded_agent_answers_local_indices(begin, count):
    """PlanInputs.shard with a non-zero begin: ranks are indices within the shard (what candidates() and materialise() take); the
    top-k's global indices minus the shard's begin are its first ranks"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = count_scene(count, shard=(begin, count))
    assert inp.shard_begin == begin
    with FrenetEngine(max_candidates=N_ROWS + 64, max_steps=inp.N) as e:
        e.plan_step(inp)
        for name in ("three_values", "nan_between", "mixed_cluster"):
            cost, flags = sp.any_plane(name, count)
            dp.write_cost_flags(e, 0, cost, flags)
            want, n_nan = hold_order(e, cost, flags, sp.SEL, sp.COL | sp.BND, what=(begin, name))
            assert len(want) == 0 or (want.min() >= 0 and want.max() < count)
            _, idx = e.topk(64)
            k = min(64, len(want) - n_nan)
            assert np.array_equal(idx[0][:k] - begin, want[:k]) and np.all(idx[0][k:] == -1)


# ---- what a sort leaves alone ----
@pytest.mark.parametrize("n", (sp.SORT_TILE + 1, sp.SORT_SMALL_MAX + 1))
def test_sort_touches_nothing_of_the_step(n):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    inp = count_scene(n)
    with FrenetEngine(max_candidates=n + 64, max_steps=inp.N) as e, FrenetEngine(max_candidates=n + 64, max_steps=inp.N) as quiet:
        res, res_q = e.plan_step(inp), quiet.plan_step(inp)
        cost, flags = e.costs()
        tk = e.topk(64)
        bytes0 = e.device_bytes
        assert bytes0 == quiet.device_bytes
        for require, exclude in sp.POOLS:
            n_pool, _ = e.sort_candidates(0, require, exclude)
            e.ranked(0, min(1, n_pool), with_cost=True)
        c2, f2 = e.costs()
        assert np.array_equal(dp.bits(c2), dp.bits(cost)) and np.array_equal(f2, flags)
        tk2 = e.topk(64)
        assert np.array_equal(dp.bits(tk2[0]), dp.bits(tk[0])) and np.array_equal(tk2[1], tk[1])
        res2 = e.plan_step(inp)                                  # the step's own result, before and after
        assert set(res) == set(res2) and all(np.array_equal(np.asarray(res[k]), np.asarray(res2[k])) for k in res if k != "kernel_ms")
        assert e.device_bytes > bytes0                           # the sort's block is counted ...
        assert quiet.device_bytes == bytes0                      # ... and a context that never sorts owns what it always did
        assert res_q["best_index"] == res["best_index"]
        grown = e.device_bytes
        e.sort_candidates(0, 0, 0)
        assert e.device_bytes == grown                           # grow-only: the same layout allocates nothing


# ---- lifetime and refusals ----
def test_lifetime_and_refusals(engines):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from frenetix_motion_planner_amd._lib import lib
    n = sp.SORT_SMALL_MAX + 1
    inp = count_scene(n)
    with FrenetEngine(max_candidates=n + 64, max_steps=inp.N) as e:
        with pytest.raises(ValueError, match=NOT_READY):         # before the first evaluated step
            e.sort_candidates()
        with pytest.raises(ValueError, match=NOT_READY):
            e.ranked(0, 1)
        e.plan_step(inp)
        for call in (lambda: e.ranked(0, 1), lambda: e.sort_view()):      # evaluated, but nothing sorted
            with pytest.raises(ValueError, match=NOT_READY):
                call()
        cost, flags = sp.any_plane("nan_between", n)
        dp.write_cost_flags(e, 0, cost, flags)
        want, _ = sp.reference_order(cost, flags, sp.COSTED, 0)
        n_pool, n_nan = e.sort_candidates()
        assert n_pool == len(want) and 0 < n_nan < n_pool < n
        for first, cnt in ((-1, 1), (0, -1), (0, n_pool + 1), (n_pool, 1), (n_pool + 1, 0), (2**62, 2**62)):
            with pytest.raises(ValueError, match=INVALID):
                e.ranked(first, cnt)
        for agent in (-1, 1):
            with pytest.raises(ValueError, match=INVALID):
                e.ranked(0, 1, agent)
            with pytest.raises(ValueError, match=INVALID):
                e.sort_candidates(agent)
        L = lib()
        a = C.c_int64(0)
        assert L.fx_sort_candidates_agent(e._ctx, 0, sp.COSTED, 0, None, C.byref(a)) == _abi.FX_ERR_INVALID_ARGUMENT
        assert L.fx_sort_candidates_batch(e._ctx, sp.COSTED, 0, C.byref(a), None) == _abi.FX_ERR_INVALID_ARGUMENT
        assert L.fx_read_ranked_agent(e._ctx, 0, 0, 1, None, None, None) == _abi.FX_ERR_INVALID_ARGUMENT
        assert L.fx_sort_views(e._ctx, 0, None, C.byref(a)) == _abi.FX_ERR_INVALID_ARGUMENT
        assert np.array_equal(e.ranked(0, n_pool), want)         # every refused call left the order readable
        assert e.last_sort_ms > 0.0
        e.plan_step(inp)                                         # a new evaluation ends the order
        for call in (lambda: e.ranked(0, 1), lambda: e.sort_view()):
            with pytest.raises(ValueError, match=NOT_READY):
                call()
        c_new, f_new = e.costs()                                 # ... and the next sort is of the new step
        assert e.sort_candidates(0, 0, 0) == (n, int(np.isnan(c_new).sum()))
        assert np.array_equal(e.ranked(0, n), sp.reference_order(c_new, f_new, 0, 0)[0])
        e.update_state(e.make_state_update(v_des=11.0))                  # a state update without an evaluation: the order is gone, no sort
        with pytest.raises(ValueError, match=NOT_READY):
            e.ranked(0, 1)
        with pytest.raises(ValueError, match=NOT_READY):
            e.sort_candidates()
