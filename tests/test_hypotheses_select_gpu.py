"""The selection of the hypotheses pass (fx_hyp_finish_kernel, fx_hyp_select_kernel) on planes a test writes:
behind a finished step the agent's raw cost rows and flag words are overwritten on the device (tests/rescore_planes.py, write_rows:
fx_device_costmap_view / fx_device_views) and restored afterwards.  For every case and every hypothesis the winner, its cost and
n_collisions must be what NumPy derives from the call's OWN returned total and collision rows under the rule
(tests/hypotheses_scene.py, numpy_selection) -- and every case asserts the property it is there for."""
import numpy as np
import pytest

from tests import device_planes as dp
from tests import hypotheses_scene as hs
from tests import rescore_planes as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stepped():
    """an engine behind a finished split step of 650 candidates with 7 obstacles, its hypotheses, its planes"""
    with hs.engine() as e:
        inp = hs.make(hs.GRIDS["mid"], 7)
        e.set_obstacle_stage(2, 3)
        res = e.plan_step(inp)
        cost, flags = e.costs()
        w = res["best_index"]
        path = tuple(e.plane(name)[:, w] for name in ("x", "y", "theta"))
        hyps = hs.hypotheses_of(inp, path)
        raw = np.ascontiguousarray(e.costmap().T)
        yield e, inp, res, raw, flags, hyps
        rp.write_rows(e, 0, raw, flags)


def answer(e, hyps, raw, flags):
    rp.write_rows(e, 0, raw, flags)
    names = list(hyps)
    r = e.hypotheses([hyps[n] for n in names], totals=True, collisions=True)
    for h, n in enumerate(names):
        g, c, k = hs.numpy_selection(r["totals"][h], r["collisions"][h], flags)
        assert r["winner"][h] == g and (dp.bits(r["cost"][h]) == dp.bits(c)) and r["n_collisions"][h] == k, (n, g, c, k)
        assert np.array_equal(np.isnan(r["totals"][h]), (flags & hs.COSTED) == 0) or np.isnan(raw).any()
        assert not r["collisions"][h][(flags & hs.SEL) == 0].any()
    return names, r


def test_the_planes_of_the_step_itself(stepped):
    e, inp, res, raw, flags, hyps = stepped
    names, r = answer(e, hyps, raw, flags)
    assert r["winner"][names.index("own")] == res["best_index"] and r["n_collisions"][names.index("own")] == res["n_collisions"]
    assert any(k > 0 for k in r["n_collisions"])


def test_boundary_flag_on_the_would_be_winner(stepped):
    e, inp, res, raw, flags, hyps = stepped
    f = flags.copy()
    f[res["best_index"]] |= hs.BND
    names, r = answer(e, hyps, raw, f)
    own = names.index("own")
    assert r["winner"][own] != res["best_index"] and r["winner"][own] >= 0
    assert r["totals"][own][r["winner"][own]] >= r["totals"][own][res["best_index"]]


def test_selectable_cleared(stepped):
    e, inp, res, raw, flags, hyps = stepped
    f = flags.copy()
    f[res["best_index"]] &= ~np.uint32(hs.SEL)
    names, r = answer(e, hyps, raw, f)
    assert r["winner"][names.index("own")] not in (-1, res["best_index"])
    # nothing selectable at all: -1, +inf, no collision counted
    f = flags & ~np.uint32(hs.SEL)
    names, r = answer(e, hyps, raw, f)
    assert np.all(r["winner"] == -1) and np.all(r["cost"] == np.inf) and np.all(r["n_collisions"] == 0)


def test_the_winner_is_the_last_candidate(stepped):
    e, inp, res, raw, flags, hyps = stepped
    n = inp.n_candidates
    last = n - 1
    assert (flags[last] & (hs.COSTED | hs.SEL)) == (hs.COSTED | hs.SEL) and n % 64 != 0      # (costed, in a tile that is not full)
    r2 = raw.copy()
    r2[:, last] = 1e-6                                    # the lowest rows of all
    names, r = answer(e, hyps, r2, flags)
    h = names.index("all_absent")
    assert r["winner"][h] == last


def test_equal_totals_go_to_the_lower_index(stepped):
    e, inp, res, raw, flags, hyps = stepped
    r2 = np.ones_like(raw)
    names, r = answer(e, hyps, r2, flags)
    h = names.index("all_absent")                      # no prediction cost, no collision: every costed total is the same number
    tot = r["totals"][h]
    assert not r["collisions"][h].any()
    el = np.nonzero(((flags & hs.SEL) != 0) & ((flags & hs.BND) == 0) & ~np.isnan(tot))[0]      # (the step's own collision flag does not count)
    assert len(el) > 100 and len(set(dp.bits(tot[el]).tolist())) == 1 and r["winner"][h] == el[0]
    own = names.index("own")                           # with the step's predictions the totals differ again
    assert len(set(dp.bits(r["totals"][own][el]).tolist())) > 1


def test_nan_and_infinite_raw_cost_rows(stepped):
    e, inp, res, raw, flags, hyps = stepped
    r2, _ = rp.plane("non_finite", inp.n_candidates, raw.shape[0])
    names, r = answer(e, hyps, r2, flags)
    own = names.index("own")
    tot = r["totals"][own][(flags & hs.COSTED) != 0]
    assert np.isnan(tot).any() and np.isinf(tot).any() and np.isfinite(tot).any()
    assert r["winner"][own] >= 0 and not np.isnan(r["cost"][own])
