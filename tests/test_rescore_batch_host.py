"""The re-score over effective cost lists and for a whole agent batch without a GPU: the entry points are
exported and declared and the ABI version stays; what the library refuses without a device; `engine.effective_cost_names` and
`rescore_weights` over the effective names; the one statement of where the responsibility term stands; the committed resource
lines; and the helpers the GPU tests build on (tests/rescore_rows.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, _lib
from frenetix_motion_planner_amd.engine import effective_cost_names, rescore_weights
from tests import rescore_planes as rp
from tests import rescore_rows as rr
from tests.test_launchers import stubbed_launchers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["distance_to_reference_path", "lateral_jerk", "longitudinal_jerk", "prediction", "velocity_offset"]


def test_entry_points_are_exported_and_declared():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    for sym in ("fx_rescore_agent_rows", "fx_rescore_batch"):
        assert hasattr(L, sym) and re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.exported_symbols()
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays
    assert "fx_launch_rescore_batch" in stubbed_launchers()   # (and declared once, nowhere weak: tests/test_launchers.py)


def test_refusals_that_need_no_device():
    L = _lib.lib()
    w, win, cost = np.ones((1, 5)), np.full(1, 7, np.int64), np.full(1, 7.0)
    agents, n_vec = np.zeros(1, np.int32), np.ones(1, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    INV = _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_rescore_agent_rows(None, 0, 1, ptr(w), None, None, ptr(win), ptr(cost), None) == INV
    assert L.fx_rescore_batch(None, 1, ptr(agents), ptr(n_vec), ptr(w), None, None, ptr(win), ptr(cost)) == INV
    assert L.fx_rescore_batch(None, -1, ptr(agents), ptr(n_vec), ptr(w), None, None, ptr(win), ptr(cost)) == INV
    assert L.fx_rescore_batch(None, 1, ptr(agents), None, None, None, None, None, None) == INV
    # no agent is no work: FX_OK, and nothing is touched -- the arrays may then be NULL
    assert L.fx_rescore_batch(None, 0, None, None, None, None, None, None, None) == _abi.FX_OK
    assert L.fx_rescore_batch(None, 0, ptr(agents), ptr(n_vec), ptr(w), None, None, ptr(win), ptr(cost)) == _abi.FX_OK
    assert win[0] == 7 and cost[0] == 7.0


def test_effective_names():
    assert effective_cost_names(NAMES) == NAMES and effective_cost_names(None, True) is None
    assert effective_cost_names(NAMES, True) == NAMES[:4] + ["responsibility", "velocity_offset"]
    assert effective_cost_names(NAMES[:4], True) == NAMES[:4] + ["responsibility"]                  # the prediction last: at the end
    assert effective_cost_names(NAMES[:3], True) == NAMES[:3] + ["responsibility"]                  # no prediction, nothing behind it
    assert effective_cost_names(NAMES[:3] + NAMES[4:], True) == NAMES[:3] + ["responsibility", "velocity_offset"]
    assert effective_cost_names([], True) == ["responsibility"]
    every = effective_cost_names(list(_abi.COST_NAMES), True)
    assert every == sorted(every) and len(every) == _abi.FX_NUM_COSTS + 1                           # its sorted place, whatever the list
    # the same place as the ids say (fx_resp_term_at) and as the tests' restatement
    for names in (NAMES, NAMES[:4], NAMES[:3], NAMES[1:2] + NAMES[4:], []):
        ids = [_abi.COST_ID[n] for n in names]
        assert effective_cost_names(names, True).index("responsibility") == rr.resp_at(ids)
    with pytest.raises(ValueError):
        effective_cost_names(NAMES + ["responsibility"], True)


def test_weights_over_the_effective_names():
    a = dict(velocity_offset=1.0, prediction=0.2, lateral_jerk=0.3, longitudinal_jerk=-0.4, distance_to_reference_path=5.0)
    b = dict(a, responsibility=2.5)
    assert rescore_weights([b], NAMES, True).tolist() == [[5.0, 0.3, -0.4, 0.2, 2.5, 1.0]]
    assert rescore_weights([a], NAMES).tolist() == [[5.0, 0.3, -0.4, 0.2, 1.0]] == rescore_weights([a], NAMES, False).tolist()
    assert rescore_weights(np.ones((3, 6)), NAMES, True).shape == (3, 6)
    for bad, resp in (([a], True), ([b], False), ([dict(b, responsibility=0.0)], True), (np.ones((3, 5)), True), (np.ones((3, 6)), False),
                      ([dict(b, responsibility=np.nan)], True)):
        with pytest.raises(ValueError):
            rescore_weights(bad, NAMES, resp)


def test_one_statement_of_where_the_term_stands():
    """the rule lives in fx_resp_term_at; the responsibility pass (fx_api_risk.hip) and the re-score (fx_api_rescore.hip) both call it"""
    src = {f: open(os.path.join(rp.CSRC, f)).read() for f in os.listdir(rp.CSRC) if f.endswith((".h", ".hip"))}
    stated = [f for f, t in src.items() if re.search(r"cost_id\[m\] > FX_COST_PREDICTION", t)]
    assert stated == ["fx_rescore_batch_plan.h"]
    for f in ("fx_api_risk.hip", "fx_api_rescore.hip"):
        assert "fx_resp_term_at(hp.cost_id, hp.n_cost)" in src[f], f


def test_committed_resource_lines():
    """profiles/rescore_batch/: every kernel of the parent with the line it had, the new kernels without scratch or spills"""
    rows = {}
    for which in ("parent", "commit"):
        with open(os.path.join(ROOT, "profiles", "rescore_batch", f"kernel_resources_{which}.txt")) as f:
            rows[which] = dict(line.split(None, 1) for line in f if line.strip())
    assert len(rows["parent"]) > 180 and all(rows["commit"].get(k) == v for k, v in rows["parent"].items())
    assert sum("fx_rescore" in k for k in rows["parent"]) == 4          # the four kernels of the per-agent pass stay
    new = {k: v for k, v in rows["commit"].items() if k not in rows["parent"]}
    assert len(new) == 4 and all("fx_rescore_batch" in k for k in new)
    for k, v in new.items():
        f = dict(zip(v.split()[0::2], (int(x) for x in v.split()[1::2])))
        assert f["scratch"] == 0 and f["spillV"] == 0 and f["spillS"] == 0, (k, v)


def test_reference_over_the_effective_list():
    """tests/rescore_rows.py on the host: the effective rows are the statement, and the reference is rescore_planes' over them"""
    rng = np.random.default_rng(5)
    ids = [_abi.COST_ID[n] for n in NAMES]
    raw, flags = rng.normal(size=(5, 30)), np.full(30, rp.OK, np.uint32)
    pred, resp = rng.normal(size=30), rng.normal(size=30)
    rows, n_pred = rr.effective_rows(raw, ids, pred, resp)
    assert n_pred == 3 and rows.shape == (6, 30)
    assert np.array_equal(rows[3], pred) and np.array_equal(rows[4], resp) and np.array_equal(rows[5], raw[4]) and np.array_equal(rows[:3], raw[:3])
    rows, n_pred = rr.effective_rows(raw[:4], ids[:4], None, resp)
    assert n_pred == 3 and np.array_equal(rows[4], resp) and np.array_equal(rows[:4], raw[:4])
    w = np.array([[0.5, -2.0, 3.0, 0.25, 1.5, 0.75]])
    for deferred in (False, True):
        _, _, tot = rr.expected(raw, flags, w, ids, deferred, pred, resp)
        for c in range(30):     # resp_sum_body (fx_risk_kernel.h) in plain Python
            s, tail = -0.0, 0.0
            terms = [w[0, 0] * raw[0, c], w[0, 1] * raw[1, c], w[0, 2] * raw[2, c], w[0, 3] * pred[c], w[0, 4] * resp[c], w[0, 5] * raw[4, c]]
            for m, t in enumerate(terms):
                if deferred and m > 3:
                    tail += t
                else:
                    s += t
            if deferred:
                s += tail
            assert tot[0][c] == 0.0 + s
    for kind in rr.EXTERNAL:
        row = rr.external_row(kind, 257, 1)
        assert row.shape == (257,) and np.array_equal(row, rr.external_row(kind, 257, 1), equal_nan=True)
    assert np.isnan(rr.external_row("non_finite", 257, 1)).any() and np.all(np.diff(rr.external_row("breaks_ties", 65, 0)) > 0)
