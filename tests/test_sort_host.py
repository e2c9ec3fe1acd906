"""The device sort (csrc/fx_sort_kernel.h) without a GPU: the sizes the GPU module is parametrised on follow
the source, its NumPy reference is Python's stable sort, the NumPy restatement of the sort key orders every plane as the reference
does, the entry points refuse what needs no device to refuse, and the planner's walk by rank on an oracle-backed engine."""
import ctypes as C

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, _lib
from tests import device_planes as dp
from tests import sort_planes as sp
from tests.oracle_engine import OracleEngine

HOST_SIZES = (1, 63, 65, 700, sp.SORT_TILE + 1, sp.SORT_SMALL_MAX + 1, 131_073)


def test_switch_sizes_follow_the_source():
    """The sizes tests/test_sort_planes.py is parametrised on, derived from the #defines of csrc/fx_sort_kernel.h: a change there
    fails here instead of leaving the GPU tests beside the switches."""
    k = sp.source_constants()
    assert k["small_max"] == sp.SORT_SMALL_MAX == 4_096                    # the largest one-workgroup agent
    assert k["tile"] == sp.SORT_TILE == k["block"] * k["items"] == 2_048
    assert k["digit_bits"] == sp.SORT_DIGIT_BITS == 8 and 64 % k["digit_bits"] == 0 and (1 << k["digit_bits"]) == k["block"]
    assert k["block"] == 256 and sp.SORT_WAVE_RUN == 64 * k["items"] == k["tile"] // (k["block"] // 64)
    assert k["key_nan"] == int(sp.KEY_NAN) and k["key_out"] == int(sp.KEY_OUT)
    # one-workgroup kernel: 24 bytes of LDS per (padded) candidate plus the counters -- comfortably inside the 160 KiB
    assert 24 * k["small_max"] + 4 * (4 * 256 + 8) <= 112 * 1024
    S, T = k["small_max"], k["tile"]
    assert {1, 63, 64, 65, T - 1, T, T + 1, S, S + 1, 3 * T - 1, 3 * T, 3 * T + 1} <= set(sp.SORT_SIZES)
    assert S + 1 > S and -(-(S + 1) // T) == 3 and (S + 1) % T == 1            # the first general agent: three tiles, the last ragged
    big = max(sp.SORT_SIZES)
    assert 90 <= -(-big // T) <= 400 and big % T != 0 and big % 64 != 0 and big <= 200_000


def test_reference_is_pythons_stable_sort():
    """reference_order against sorted(pool, key=cost.__getitem__) where no pool member is NaN (Python's sort has no defined answer
    with NaNs), and against device_planes.lex_order for the survivor pool with the NaNs cut off"""
    checked = 0
    for name in sp.ALL_PLANES:
        for n in (1, 63, 65, 700):
            cost, flags = sp.any_plane(name, n)
            for require, exclude in sp.POOLS:
                ids, n_nan = sp.reference_order(cost, flags, require, exclude)
                pool = [g for g in range(n) if (int(flags[g]) & require) == require and (int(flags[g]) & exclude) == 0]
                assert sorted(ids.tolist()) == pool and n_nan == sum(1 for g in pool if cost[g] != cost[g])
                if n_nan == 0:
                    assert ids.tolist() == sorted(pool, key=cost.__getitem__), (name, n, require)
                    checked += 1
                else:   # NaNs last, in index order among themselves; the rest is Python's order of the rest
                    rest = [g for g in pool if cost[g] == cost[g]]
                    assert ids.tolist() == sorted(rest, key=cost.__getitem__) + [g for g in pool if cost[g] != cost[g]], (name, n, require)
            ids, n_nan = sp.reference_order(cost, flags, sp.SEL, sp.COL | sp.BND)
            want, want_c = dp.lex_order(cost, flags)
            assert np.array_equal(ids[:len(ids) - n_nan], want) and np.array_equal(dp.bits(cost[ids[:len(ids) - n_nan]]), dp.bits(want_c))
    assert checked > 100


def test_key_orders_every_plane_as_the_reference():
    """fx_sort_key restated in NumPy: a stable sort of the keys, and eight stable passes over their bytes, give the reference's
    order; ranks [0, n_pool) are the pool"""
    for name in sp.ALL_PLANES:
        for n in HOST_SIZES:
            cost, flags = sp.any_plane(name, n)
            for require, exclude in sp.POOLS:
                ids, n_nan = sp.reference_order(cost, flags, require, exclude)
                keys = sp.sort_keys(cost, flags, require, exclude)
                order = np.argsort(keys, kind="stable")
                assert np.array_equal(order[:len(ids)], ids), (name, n, require)
                assert int((keys == sp.KEY_NAN).sum()) == n_nan and int((keys != sp.KEY_OUT).sum()) == len(ids)
                if n <= sp.SORT_SMALL_MAX + 1:
                    assert np.array_equal(sp.radix_order(keys), order), (name, n, require)


def test_key_of_the_special_values():
    cost = np.array([-np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan, -np.nan])
    keys = sp.sort_keys(cost, np.zeros(len(cost), np.uint32), 0, 0)
    assert keys[3] == keys[4] and np.all(np.diff(keys[[0, 1, 2, 3, 5, 6, 7, 8]].astype(object)) > 0)
    assert keys[7] == np.uint64(0xFFF0000000000000) and keys[8] == keys[9] == sp.KEY_NAN
    nan = dp._nan_payloads(np.random.default_rng(3), 1000)
    assert np.all(sp.sort_keys(nan, np.zeros(1000, np.uint32), 0, 0) == sp.KEY_NAN)
    assert np.all(sp.sort_keys(nan, np.zeros(1000, np.uint32), sp.SEL, 0) == sp.KEY_OUT)


def test_planes_are_what_their_names_say():
    for n in (65, sp.SORT_SMALL_MAX + 1):
        for k in range(8):
            cost, flags = sp.extra_plane(f"byte_{k}", n)
            keys = sp.sort_keys(cost, np.zeros(n, np.uint32), 0, 0)
            diff = np.bitwise_or.reduce(keys ^ keys[0])
            assert diff != 0 and (int(diff) & ~(0xFF << (8 * k))) == 0, (k, hex(int(diff)))      # only byte k differs
            c2, f2 = sp.extra_plane(f"byte_{k}", n)
            assert np.array_equal(dp.bits(cost), dp.bits(c2)) and np.array_equal(flags, f2)      # seeded
        keys = sp.sort_keys(sp.extra_plane("digits_0_255", n)[0], np.zeros(n, np.uint32), 0, 0)
        for k in range(8):
            seen = set(((keys >> np.uint64(8 * k)) & np.uint64(0xFF)).tolist())
            assert {0, 255} <= seen, (k, seen)
        cost, _ = sp.extra_plane("one_bucket_but_one", n)
        assert np.count_nonzero(cost != 1.5) == 1
        cost, _ = sp.extra_plane("descending", n)
        assert np.all(np.diff(cost) < 0) and cost[0] > 0 > cost[-1]
        cost, _ = sp.extra_plane("signs_interleaved", n)
        z = np.nonzero(cost == 0.0)[0]
        assert np.any(np.signbit(cost[z])) and np.any(~np.signbit(cost[z])) and np.any(np.diff(z) == 1) and np.any(np.abs(cost[cost != 0]) < 1e-300)
        cost, flags = sp.extra_plane("nan_between", n)
        nan = np.isnan(cost)
        assert nan.any() and np.signbit(cost[nan]).any() and (~np.signbit(cost[nan])).any() and len(set(dp.bits(cost[nan]).tolist())) > 10
        for require, exclude in sp.POOLS:      # every pool a proper, non-empty subset with NaNs in it
            m = sp.pool_mask(flags, require, exclude)
            assert 0 < m.sum() and (m.sum() < n or (require, exclude) == (0, 0)) and np.isnan(cost[m]).any()


def test_refusals_that_need_no_device():
    """a NULL context is refused by every new entry point; the Python layer refuses what the library would"""
    L = _lib.lib()
    a, b = C.c_int64(7), C.c_int64(7)
    p = C.c_void_p(5)
    idx = np.zeros(4, np.int64)
    assert L.fx_sort_candidates_agent(None, 0, sp.COSTED, 0, C.byref(a), C.byref(b)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"NULL" in L.fx_last_error()
    assert L.fx_sort_candidates_batch(None, sp.COSTED, 0, C.byref(a), C.byref(b)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_read_ranked_agent(None, 0, 0, 4, idx.ctypes.data, None, None) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_sort_views(None, 0, C.byref(p), C.byref(a)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_last_sort_ms(None) == -1.0
    assert (a.value, b.value, p.value) == (7, 7, 5) and not idx.any()          # nothing was written
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15                     # additive: the version stays
    for name in ("fx_sort_candidates_agent", "fx_sort_candidates_batch", "fx_read_ranked_agent", "fx_sort_views", "fx_last_sort_ms"):
        assert name in _lib.exported_symbols()


# ------------------------------------------------------------------------------------------------ the planner's walk by rank
class RankedOracleEngine(OracleEngine):
    """OracleEngine with the engine's order-by-rank surface, answered from the oracle's costs"""

    def __init__(self):
        super().__init__()
        self.orders, self.sorts, self.reads = {}, [], []

    def plan_step(self, inp):
        self.orders = {}
        return super().plan_step(inp)

    def sort_candidates(self, agent=0, require=_abi.FX_FLAG_COSTED, exclude=0):
        out = self.last[agent][1]
        ids, n_nan = sp.reference_order(out["cost"], out["flags"], require, exclude)
        self.orders[agent] = ids
        self.sorts.append((agent, require, exclude))
        return len(ids), n_nan

    def ranked(self, first, n, agent=0, with_cost=False):
        ids = self.orders.get(agent)
        if ids is None:
            raise ValueError(f"fxplan: no valid order (status {_abi.FX_ERR_NOT_READY})")
        if first < 0 or n < 0 or first + n > len(ids):
            raise ValueError(f"fxplan: ranks outside the pool (status {_abi.FX_ERR_INVALID_ARGUMENT})")
        self.reads.append((first, n))
        ids = ids[first:first + n].copy()
        out = self.last[agent][1]
        return (ids, out["cost"][ids].copy(), out["flags"][ids].copy()) if with_cost else ids


def _planner(engine, **cfg):
    from tests.test_retained_samples import make_planner
    return make_planner(engine, **cfg)


def _survivor_order(engine):
    out = engine.last[0][1]
    ids, n_nan = sp.reference_order(out["cost"], out["flags"], sp.SEL, sp.COL | sp.BND)
    return ids[:len(ids) - n_nan]


@pytest.fixture
def sort_any_size(monkeypatch):
    """ranked_ids goes to the engine's `ranked` whatever the candidate count (the planner's steps lie below the measured switch)"""
    from frenetix_motion_planner_amd import trajectories
    monkeypatch.setattr(trajectories, "DEVICE_SORT_MIN_CANDIDATES", 0)


def test_ranked_ids_keeps_the_host_path_below_the_switch_size():
    """a planner-sized step lies below DEVICE_SORT_MIN_CANDIDATES: the walk by rank gives the same answer from the host arrays and
    the engine is never asked to sort"""
    from frenetix_motion_planner_amd import trajectories
    assert trajectories.DEVICE_SORT_MIN_CANDIDATES == 13_000
    eng = RankedOracleEngine()
    rp = _planner(eng, device_sort=True)
    seen = []

    def check(traj):
        seen.append(traj.uniqueId)
        return 0.7 if len(seen) <= 70 else 0

    rp.road_boundary_check = check
    assert rp.plan() is not None and rp.last_step.n_candidates < trajectories.DEVICE_SORT_MIN_CANDIDATES
    order = _survivor_order(eng)
    assert rp.optimal_trajectory.uniqueId == order[70] and seen == order[:71].tolist()
    want, _ = sp.reference_order(eng.last[0][1]["cost"], eng.last[0][1]["flags"], sp.COSTED, 0)
    assert len(rp.all_traj) == len(want) and [rp.all_traj._id_at(j) for j in range(len(want))] == want.tolist()
    assert not eng.sorts and not eng.reads
    rp.close()


@pytest.mark.parametrize("n_reject", (16, 70))
def test_walk_continues_past_the_survivors(n_reject, sort_any_size):
    """A road_boundary_check that rejects the first 16, then the first 70, survivors: the default planner has walked its 16 and
    takes the fallback, as it does today; with device_sort it goes on by rank and returns the first accepted candidate."""
    picked = {}
    for device_sort in (False, True):
        eng = RankedOracleEngine()
        rp = _planner(eng, device_sort=device_sort)
        seen = []

        def check(traj):
            seen.append(traj.uniqueId)
            return 0.7 if len(seen) <= n_reject else 0

        rp.road_boundary_check = check
        pair = rp.plan()
        order = _survivor_order(eng)
        assert len(order) > n_reject + 1
        if device_sort:
            assert pair is not None and rp.optimal_trajectory.uniqueId == order[n_reject]
            assert seen == order[:n_reject + 1].tolist()
            assert (0, sp.SEL, sp.COL | sp.BND) in eng.sorts and eng.reads[0][0] == 16      # the ranks behind the top-k's page
            for g in order[:n_reject]:
                t = rp.last_step.sample(int(g))
                assert t.boundary_harm == 0.7 and t._coll_detected is False
            assert rp.optimal_trajectory.boundary_harm == 0 and rp._collision_counter == eng.last[0][1]["result"]["n_collisions"]
        else:
            assert pair is None and rp.optimal_trajectory is None and seen == order[:16].tolist()
            assert not eng.sorts and not eng.reads
        picked[device_sort] = seen
        rp.close()
    assert picked[True][:16] == picked[False]


def test_device_sort_changes_nothing_where_the_default_finds_one(sort_any_size):
    """no rejecting check, and a check that rejects three: the identical trajectory, and no sort at all"""
    for reject in (0, 3):
        got = []
        for device_sort in (False, True):
            eng = RankedOracleEngine()
            rp = _planner(eng, device_sort=device_sort)
            seen = []

            def check(traj):
                seen.append(traj.uniqueId)
                return 0.7 if len(seen) <= reject else 0

            rp.road_boundary_check = check
            assert rp.plan() is not None
            got.append((rp.optimal_trajectory.uniqueId, list(seen), rp._collision_counter))
            assert not eng.sorts
            rp.close()
        assert got[0] == got[1]


def test_all_traj_pages_through_ranks(sort_any_size):
    """all_traj with device_sort: the length is the pool's size, items come by rank in pages, the C costs are never read"""
    from frenetix_motion_planner_amd import reactive_planner as rpm
    eng = RankedOracleEngine()
    calls = []
    eng.costs = lambda agent=0: calls.append(agent) or OracleEngine.costs(eng, agent)
    rp = _planner(eng, device_sort=True)
    assert rp.plan() is not None
    calls.clear()                                                  # (an oracle-backed sample, the winner, reads the step's arrays)
    out = eng.last[0][1]
    want, _ = sp.reference_order(out["cost"], out["flags"], sp.COSTED, 0)
    lst = rp.all_traj
    assert len(lst) == len(want) == out["result"]["n_returned"]
    assert [lst._id_at(j) for j in range(len(lst))] == want.tolist()
    assert not calls and eng.sorts == [(0, sp.COSTED, 0)]          # (the list itself: ranks only)
    assert [t.uniqueId for t in lst[:5]] == want[:5].tolist() and lst[-1].uniqueId == want[-1] and lst[7].uniqueId == want[7]
    assert [t.uniqueId for t in lst] == want.tolist()
    assert all(n <= rpm.SORTED_PAGE and first % rpm.SORTED_PAGE == 0 for first, n in eng.reads)
    with pytest.raises(IndexError):
        lst[len(want)]
    ids = rp.last_step.ranked_ids(3, 10)
    assert np.array_equal(ids, want[3:13]) and np.array_equal(rp.last_step.ranked_ids(len(want) - 2, 10), want[-2:])
    assert np.array_equal(rp.last_step.sorted_ids(), want)          # (the host path: reads the costs, same order)
    rp.close()


def test_ranked_ids_answers_from_the_host_arrays_of_a_stale_step(sort_any_size):
    eng = RankedOracleEngine()
    rp = _planner(eng, device_sort=True)
    pair = rp.plan()
    step = rp.last_step
    want = step.sorted_ids()                       # (the arrays are on the host from here on)
    n_sorts = len(eng.sorts)
    cart, cl, lon, lat = pair
    rp.update_externals(x_0=cart[1], x_cl=(lon[1], lat[1]), desired_velocity=11.0)
    assert rp.plan() is not None and step._stale
    assert np.array_equal(step.ranked_ids(0, 50), want[:50]) and step.ranked_count()[0] == len(want)
    assert len(eng.sorts) == n_sorts               # nothing was sorted for the stale step
    rp.close()
