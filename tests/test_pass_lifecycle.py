"""The passes beside the plan step share one host scaffold (csrc/fx_pass.h): the layout of a device block, the grow-only block, the
event pair of a pass's device time, "the inputs are the last evaluation's".  This file holds the scaffold to what the passes' own
copies of it did: on one engine the passes run interleaved on lists of 70, 7 and 120 candidates -- the blocks are reused at three
layouts -- and every output of every call equals, bit for bit, the output of the same call on a fresh engine that planned the same
step and made only that call (for a select-only step: behind the materialise call that the pass reads from).

Shapes: 5 x 5 x 5 = 125 candidates (one full tile of 64 and a ragged one) and 3 x 3 x 5 = 45 (below one tile), N = 10 steps, two
obstacles in the step and two in the risk tables, a cost list with the prediction term, the cost map stored; once with the bundle
and once select-only, where the passes read the sparse set.  draw_traj_set keeps every candidate's rows defined, so any index may
be listed; about half of the candidates are selectable.  The lists of the 45-candidate step hold duplicates (70 and 120 entries).

Accounting.  Every block grows to its largest call and never shrinks, and a block that grows gives back what it held: after the
three rounds the engine owns exactly what a fresh engine owns after the 120 round alone (the layouts grow with the list), the 7
round changes nothing, a second 120 round changes nothing, and an engine that never calls a pass owns what it owned after its step.

Refusals.  Behind a state update and before the next evaluation every pass that reads the step's inputs, its cost planes or a sparse
set is refused with FX_ERR_NOT_READY and allocates nothing: all of them after a select-only step; after a step with the bundle
risk() and risk_costs() read only the stored planes of the last evaluation, are not refused by the library and are left out here.
Every refusal asked for is a check on the host; nothing here can fault."""
import dataclasses
import re

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests.test_risk_costs_gpu import WEIGHTS, _same
from tests.test_risk_gpu import BASE, EGO, HARM, _predictions

pytestmark = pytest.mark.gpu

NOT_READY = re.escape(f"(status {_abi.FX_ERR_NOT_READY})")
ROUNDS = (70, 7, 120)
CALLS = ("materialise", "risk", "risk_costs", "prediction_probability", "sort")


def _inputs(grid, bundle):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    n_t = grid[0]
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(n_t, grid[1], grid[2] - 1), n_obstacles=2,
                                horizon=1.0, n_pred=10, draw_traj_set=True, write_bundle=bundle, write_costmap=True,
                                cost_weights=dict(synthetic.DEFAULT_COST_WEIGHTS, prediction=0.2))
    # N = 10: end times on the last n_t steps of the horizon, lateral offsets a vehicle reaches within a second (d0 = 0.2 last)
    inp = dataclasses.replace(inp, t_samp=np.arange(10 - n_t + 1, 11) * inp.dt, d_samp=np.append(np.linspace(-0.3, 0.3, grid[2] - 1), 0.2))
    assert inp.N == 10 and inp.n_candidates == grid[0] * grid[1] * grid[2] and "prediction" in inp.cost_names
    return inp


def _planned(inp, update=None):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=inp.n_candidates, device=0)
    e.plan_step(inp)
    if update is not None:
        e.update_state(update)
        e.step_raw()
    return e


def _lists(C_):
    rng = np.random.default_rng(5)
    return {n: (rng.choice(C_, n, replace=False) if n <= C_ else rng.integers(0, C_, n)).astype(np.int64) for n in ROUNDS}


@pytest.fixture(scope="module", params=[(5, 5, 5), (3, 3, 5)], ids=["125", "45"])
def tables(request):
    """the risk tables of the grid's step: obstacles along the candidates of the step WITH the bundle, for both of its forms"""
    from frenetix_motion_planner_amd import risk
    inp = _inputs(request.param, True)
    with _planned(inp) as e:
        _, flags = e.costs()
        planes = {n: e.plane(n).T.copy() for n in ("x", "y", "theta", "v")}
    assert (flags & _abi.FX_FLAG_COSTED).all() and 0 < ((flags & _abi.FX_FLAG_SELECTABLE) != 0).sum() < len(flags)
    preds, typ = _predictions(planes, flags, np.random.default_rng(3), n_obs=2)
    return request.param, risk.obstacle_tables(preds, typ)


def _call(e, name, ids, bundle, alone):
    """one pass on the listed candidates; alone: on an engine that has made no other call -- a select-only step's passes read the
    sparse set, so the materialise call they depend on comes first"""
    from frenetix_motion_planner_amd import risk
    params = risk.risk_params(BASE, HARM, **EGO)
    if alone and not bundle and name in ("risk", "risk_costs", "prediction_probability"):
        e.materialise(ids)
    if name == "materialise":
        return e.materialise(ids)
    if name == "risk":
        return e.risk(params, ids)
    if name == "risk_costs":
        return e.risk_costs(params, risk.risk_cost_params(WEIGHTS), ids)
    if name == "prediction_probability":
        return e.prediction_probability(EGO["ego_length"], EGO["ego_width"], ids=ids, per_obstacle=True)
    n_pool, n_nan = e.sort_candidates()
    return (n_pool, n_nan) + tuple(e.ranked(0, min(len(ids), n_pool), with_cost=True))


def _timers(e):
    return dict(risk=e.last_risk_ms, prediction_probability=e.last_predprob_ms, sort=e.last_sort_ms, materialise=e.last_materialise_ms)


@pytest.mark.parametrize("bundle", [True, False], ids=["bundle", "select_only"])
def test_interleaved_passes_equal_fresh_engines(tables, bundle):
    grid, tabs = tables
    inp = _inputs(grid, bundle)
    lists = _lists(inp.n_candidates)
    update = None

    alone = {}   # computed once per call, left unchanged

    def fresh(name, ids, upd=None):
        key = (name, len(ids), upd is None)
        if key not in alone:
            with _planned(inp, upd) as e:
                assert e.device_bytes == bytes0
                e.set_risk_obstacles(tabs)
                alone[key] = _call(e, name, ids, bundle, alone=True)
        return alone[key]

    eng, twin = _planned(inp), _planned(inp)
    try:
        bytes0 = eng.device_bytes
        assert twin.device_bytes == bytes0
        assert _timers(eng) == dict.fromkeys(_timers(eng), -1.0)   # before the first pass of each kind
        eng.set_risk_obstacles(tabs)

        def round_(ids, upd=None):
            sizes = []
            for name in CALLS:
                got = _call(eng, name, ids, bundle, alone=False)
                assert _same(got, fresh(name, ids, upd)), (name, len(ids))
                sizes.append(eng.device_bytes)
            assert sizes == sorted(sizes)
            return sizes[-1]

        after = {n: round_(lists[n]) for n in ROUNDS}
        for name, ms in _timers(eng).items():
            assert np.isfinite(ms) and ms > 0, name
        assert after[70] > bytes0 and after[7] == after[70] and after[120] >= after[70]   # grow-only
        assert round_(lists[120]) == after[120]
        with _planned(inp) as e:   # every block holds its largest call and nothing else: the 120 round alone
            e.set_risk_obstacles(tabs)
            for name in CALLS:
                _call(e, name, lists[120], bundle, alone=False)
            assert e.device_bytes == after[120]
        assert np.nanmax(alone[("risk_costs", 120, True)]["obst_risk_max"]) > 0   # (not a comparison of zeros)

        # behind a state update the inputs are another step's: refused on the host, nothing allocated
        update = eng.make_state_update(v_des=11.0)
        eng.update_state(update)
        refused = [n for n in CALLS if not (bundle and n in ("risk", "risk_costs"))]
        for name in refused:
            with pytest.raises(ValueError, match=NOT_READY):
                _call(eng, name, lists[7], bundle, alone=False)
        with pytest.raises(ValueError, match=NOT_READY):
            eng.ranked(0, 1)
        assert eng.device_bytes == after[120]
        eng.step_raw()
        with pytest.raises(ValueError, match=NOT_READY):   # the order of the step before
            eng.ranked(0, 1)
        assert round_(lists[7], update) == after[120]   # the next step: every pass works again
        twin.update_state(update)
        twin.step_raw()
        assert twin.device_bytes == bytes0
    finally:
        eng.close()
        twin.close()
