"""The re-score over effective cost lists (fx_rescore_agent_rows, csrc/fx_rescore_batch_kernel.h) on raw cost
rows, flag planes AND external rows written by the test (tests/rescore_planes.py, tests/rescore_rows.py): candidates n = 1, 63, 64,
65 (a wave), 257 (a tile and one); vectors W = 1, 63, 64, 65 -- both sides of the regime switch.  Every call runs in the regime the
rule chooses and in the forced other one, with and without totals.

Reference: NumPy over the effective list -- the step's rows with `pred` in place of the prediction's row and `resp` inserted in
front of the first term behind the prediction -- fx_cost_sum.h operation by operation with n_cost := n_eff (rescore_planes.totals_of;
the library is built with -ffp-contract=off).  winner equal, cost and totals BIT for bit, any NaN standing for any NaN.

Scenes: the undeferred form (the obstacle stage inside the walk), the deferred form (the obstacle kernel closed the sum: the inserted
term joins the tail, which is then never empty) and a list whose last entry is the prediction, so `resp` lands at the end."""
import ctypes as C

import numpy as np
import pytest

from tests import device_planes as dp
from tests import rescore_planes as rp
from tests import rescore_rows as rr

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 257)
N_VECS = (1, 63, 64, 65)
ROWS = ((True, False), (False, True), (True, True))   # (pred, resp) given


@pytest.fixture(scope="module")
def engines():
    """one engine per (scene kind, candidate count), each behind one finished step that stored its cost map"""
    from frenetix_motion_planner_amd._lib import lib
    from frenetix_motion_planner_amd.engine import FrenetEngine
    made = {}

    def get(kind, n):
        if (kind, n) not in made:
            inp = rr.scene(n, kind)
            e = FrenetEngine(max_candidates=n + 64, max_steps=inp.N)
            e.set_obstacle_stage(2 if kind == "deferred" else 1)
            e.plan_step(inp)
            made[(kind, n)] = (e, inp, bool(e.step_info()["obstacle_kernel"]))
        return made[(kind, n)]

    yield get
    lib().fx_rescore_set_regime(0)
    for e, _, _ in made.values():
        e.close()


def hold(e, inp, deferred, raw, flags, W, pred, resp, what):
    """rescore(W, pred, resp) with and without totals, in the rule's regime and in the other one, against the reference"""
    from frenetix_motion_planner_amd._lib import lib
    win, cost, tot = rr.expected(raw, flags, W, inp._cost_id, deferred, pred, resp)
    try:
        for regime in (0, rp.LANE, rp.VECTOR):
            lib().fx_rescore_set_regime(regime)
            for totals in (False, True):
                r = e.rescore(W, totals=totals, pred=pred, resp=resp)
                rr.same_result(r, win, cost, (what, regime, totals))
                assert not np.isnan(r["cost"]).any() and np.all((r["winner"] >= 0) | (r["cost"] == np.inf))
                assert (r["totals"] is None) if not totals else rp.same_nan_or_bits(r["totals"], tot), (what, regime)
    finally:
        lib().fx_rescore_set_regime(0)
    return win, cost, tot


def weights(n_vec, n_eff):
    return rp.weight_vectors(n_vec, n_eff)


def test_the_forms_the_scenes_are_for(engines):
    _, inp, deferred = engines("plain", 257)
    assert not deferred and inp.cost_names[-1] == "velocity_offset" and rr.resp_at(inp._cost_id) == len(inp.cost_names) - 1
    _, inp, deferred = engines("deferred", 257)
    assert deferred and rr.resp_at(inp._cost_id) == inp.cost_names.index("prediction") + 1
    _, inp, deferred = engines("pred_last", 257)
    assert inp.cost_names[-1] == "prediction" and rr.resp_at(inp._cost_id) == len(inp.cost_names)


@pytest.mark.parametrize("kind", rr.SCENES)
@pytest.mark.parametrize("n", SIZES)
def test_external_rows_on_written_planes(kind, n, engines):
    e, inp, deferred = engines(kind, n)
    n_cost = len(inp.cost_names)
    for name, ext in (("flag_reasons", "plain"), ("non_finite", "plain"), ("last_wins", "non_finite"), ("nothing_eligible", "plain")):
        raw, flags = rp.plane(name, n, n_cost)
        rp.write_rows(e, 0, raw, flags)
        for n_vec in N_VECS:
            for has_pred, has_resp in ROWS:
                pred = rr.external_row(ext, n, 1) if has_pred else None
                resp = rr.external_row(ext, n, 2) if has_resp else None
                W = weights(n_vec, n_cost + int(has_resp))
                win, cost, tot = hold(e, inp, deferred, raw, flags, W, pred, resp, (kind, n, name, ext, n_vec, has_pred, has_resp))
                if name == "nothing_eligible":
                    assert np.all(win == -1) and np.all(cost == np.inf)
                if ext == "non_finite" and n >= 63:
                    assert np.isnan(tot).any() and np.isinf(tot).any()


@pytest.mark.parametrize("kind", rr.SCENES)
@pytest.mark.parametrize("n", SIZES)
def test_ties_only_the_external_row_breaks(kind, n, engines):
    """every candidate has the same rows of its own: the external row alone orders them -- ascending with the index, so the lowest
    eligible index wins under a positive weight of that row and the highest under a negative one"""
    e, inp, deferred = engines(kind, n)
    n_cost = len(inp.cost_names)
    raw, flags = rp.plane("all_equal", n, n_cost)
    raw[:] = np.floor(raw * 8.0) / 8.0          # (multiples of 1/8: every sum below is exact)
    rp.write_rows(e, 0, raw, flags)
    first, last = n // 3, n - 1                 # (the plane's first n // 3 candidates collide)
    for has_pred, has_resp in ROWS:
        row = rr.external_row("breaks_ties", n, 0)
        same = np.full(n, 0.25)
        pred = (same if has_resp else row) if has_pred else None
        resp = row if has_resp else None
        k = rr.resp_at(inp._cost_id) if has_resp else inp.cost_names.index("prediction")
        for n_vec in N_VECS:
            W = np.ones((n_vec, n_cost + int(has_resp)))
            W[1::2, k] = -1.0
            win, _, tot = hold(e, inp, deferred, raw, flags, W, pred, resp, (kind, n, n_vec, has_pred, has_resp))
            assert np.all(win[0::2] == first) and np.all(win[1::2] == last)
            # without the row the candidates tie: the step's own rows answer the lowest index under every vector
            if not has_pred:
                r = e.rescore(np.delete(W, k, axis=1))
                assert np.all(r["winner"] == first)


@pytest.mark.parametrize("n", SIZES)
def test_without_rows_it_is_the_per_agent_call(n, engines):
    """fx_rescore_agent_rows with both rows NULL against fx_rescore_agent: every output, in both regimes"""
    from frenetix_motion_planner_amd._lib import check, lib
    for kind in ("plain", "deferred"):
        e, inp, _ = engines(kind, n)
        n_cost = len(inp.cost_names)
        raw, flags = rp.plane("non_finite", n, n_cost)
        rp.write_rows(e, 0, raw, flags)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        try:
            for regime in (0, rp.LANE, rp.VECTOR):
                lib().fx_rescore_set_regime(regime)
                for n_vec in N_VECS:
                    W = weights(n_vec, n_cost)
                    want = e.rescore(W, totals=True)
                    win, cost, tot = np.full(n_vec, -7, np.int64), np.full(n_vec, -7.0), np.full((n_vec, n), -7.0)
                    check(lib().fx_rescore_agent_rows(e._ctx, 0, n_vec, ptr(W), None, None, ptr(win), ptr(cost), ptr(tot)))
                    rr.same_result(dict(winner=win, cost=cost), want["winner"], want["cost"], (kind, n, regime, n_vec))
                    assert rp.same_nan_or_bits(tot, want["totals"])
                    got = e.rescore_batch([W])[0]
                    rr.same_result(got, want["winner"], want["cost"], (kind, n, regime, n_vec, "batch of one"))
        finally:
            lib().fx_rescore_set_regime(0)
