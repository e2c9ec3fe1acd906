"""The re-score kernels (csrc/fx_rescore_kernel.h) on raw cost rows and flag planes written by the test
(tests/rescore_planes.py), at the sizes where the pass changes its code path: candidates n = 1, 63, 64, 65 (a wave), 257 (a tile of
256 and one), 4 097 (17 tiles, the last of ONE candidate; 129 slices in the vector regime); vectors W = 1, 63, 64, 65 -- both sides of
the regime switch FX_RESCORE_VECTOR_MIN = 64 and of a wave of vectors (tests/test_rescore_plan.py derives the sizes from the source).

Reference: NumPy on the written planes -- fx_cost_sum.h operation by operation (the library is built with -ffp-contract=off, NumPy
fuses nothing: one IEEE operation per operation on both sides), NaN without FX_FLAG_COSTED, the lexsort minimum of the eligible
candidates.  winner is compared for equality, cost and totals BIT for bit; where both sides hold a NaN any NaN stands for any (inf - inf
carries the sign the hardware gives it; a NaN is never a winner's cost).  Every call is made in the regime the rule chooses and in the
other one (`fx_rescore_set_regime`): the bits do not depend on it."""
import numpy as np
import pytest

from tests import device_planes as dp
from tests import rescore_planes as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """one engine per candidate count, each behind one finished step that stored its cost map"""
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    made = {}

    def get(n):
        if n not in made:
            inp = rp.count_scene(n)
            e = FrenetEngine(max_candidates=n + 64, max_steps=inp.N)
            e.plan_step(inp)
            made[n] = (e, inp)
        return made[n]

    yield get
    lib().fx_rescore_set_regime(0)
    for e, _ in made.values():
        e.close()


def hold(e, inp, raw, flags, W, what):
    """rescore(W) with and without totals, in the rule's regime and in the other one, against the reference"""
    from frenetix_motion_planner_amd._lib import lib
    n_pred = inp.cost_names.index("prediction")
    deferred = bool(e.step_info()["obstacle_kernel"])
    win, cost, tot = rp.expected(raw, flags, W, n_pred, deferred)
    n = raw.shape[1]
    chosen = lib().fx_rescore_regime(n, len(W))
    assert chosen == (rp.VECTOR if len(W) >= rp.VECTOR_MIN else rp.LANE)
    try:
        for regime in (0, rp.LANE, rp.VECTOR):
            lib().fx_rescore_set_regime(regime)
            assert lib().fx_rescore_regime(n, len(W)) == (regime or chosen)
            for totals in (False, True):
                r = e.rescore(W, totals=totals)
                bad = np.nonzero(r["winner"] != win)[0]
                assert len(bad) == 0, (what, regime, totals, bad[:4], r["winner"][bad[:4]], win[bad[:4]], r["cost"][bad[:4]], cost[bad[:4]])
                assert np.array_equal(dp.bits(r["cost"]), dp.bits(cost)), (what, regime, totals)
                assert not np.isnan(r["cost"]).any() and np.all((r["winner"] >= 0) | (r["cost"] == np.inf))
                if totals:
                    assert rp.same_nan_or_bits(r["totals"], tot), (what, regime)
                else:
                    assert r["totals"] is None
    finally:
        lib().fx_rescore_set_regime(0)
    return win, cost, tot


def test_the_reference_fuses_nothing():
    assert rp.contraction_is_off()


def test_written_rows_read_back_bit_for_bit(engines):
    e, inp = engines(65)
    raw, flags = rp.plane("non_finite", 65, len(inp.cost_names))
    rp.write_rows(e, 0, raw, flags)
    assert np.array_equal(dp.bits(e.costmap()), dp.bits(raw.T)) and np.array_equal(e.costs()[1], flags)
    _, ld, n_cost = rp.costmap_view(e)
    assert ld >= 65 and ld % 64 == 0 and n_cost == len(inp.cost_names) == 5


@pytest.mark.parametrize("n", rp.SIZES)
def test_rescore_on_written_planes(n, engines):
    e, inp = engines(n)
    n_cost = len(inp.cost_names)
    for name in rp.PLANES:
        raw, flags = rp.plane(name, n, n_cost)
        rp.write_rows(e, 0, raw, flags)
        for n_vec in rp.N_VECS:
            W = rp.weight_vectors(n_vec, n_cost)
            win, cost, tot = hold(e, inp, raw, flags, W, (n, name, n_vec))
            # the planes are what their names say
            if name == "all_equal":
                assert np.all(win == n // 3)
            elif name == "ties_under_some" and n > 1:
                assert win[0] == n // 3 and tot[0][n // 3] == tot[0][n - 1] and (n_vec == 1 or (win[1] == n - 1 and tot[1][n // 3] != tot[1][n - 1]))
            elif name == "nothing_eligible":
                assert np.all(win == -1) and np.all(cost == np.inf)
            elif name == "flag_reasons" and n >= 63:
                losers = {(j * (n // 3) + n // 7) % n for j in range(3)}
                assert len(losers) == 3 and int(np.nanargmin(tot[0])) in losers and win[0] not in losers
            elif name == "last_wins":
                assert win[0] == n - 1
            elif name == "non_finite" and n >= 63:
                assert np.isnan(tot).any() and np.isinf(tot).any()


def test_infinite_totals_take_part(engines):
    """only +inf totals are eligible: infinite is still a candidate, and the lowest index among them wins in both regimes"""
    n = 257
    e, inp = engines(n)
    n_cost = len(inp.cost_names)
    raw, flags = rp.plane("last_wins", n, n_cost)
    flags[:] = rp.SEL | rp.COL | rp.COSTED
    at = np.array([70, 200, 256])
    flags[at] = rp.OK
    raw[2, at] = np.inf
    rp.write_rows(e, 0, raw, flags)
    W = np.abs(rp.weight_vectors(65, n_cost))
    win, cost, _ = hold(e, inp, raw, flags, W, "only_inf")
    assert np.all(win == 70) and np.all(cost == np.inf)
