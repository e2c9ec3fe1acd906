"""The re-score pass without a GPU: the entry points are exported and declared and the ABI version stays
(additive, as sections 15 to 22 were); the argument handling of FrenetEngine.rescore (`engine.rescore_weights`: dicts -> array in
cost_names order, the ValueError cases, shapes); what the library refuses without a device; the committed resource lines name the new
kernels without scratch; and the helpers the GPU tests build on (tests/rescore_planes.py) hold what they claim on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, _lib
from frenetix_motion_planner_amd.engine import rescore_weights
from tests import device_planes as dp
from tests import rescore_planes as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["distance_to_reference_path", "lateral_jerk", "longitudinal_jerk", "prediction", "velocity_offset"]


def test_entry_points_are_exported_and_declared():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    for sym in ("fx_rescore_agent", "fx_last_rescore_ms", "fx_device_costmap_view"):
        assert hasattr(L, sym) and re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.exported_symbols()
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays


def test_refusals_that_need_no_device():
    L = _lib.lib()
    w, win, cost = np.ones((1, 5)), np.zeros(1, np.int64), np.zeros(1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.fx_rescore_agent(None, 0, 1, ptr(w), ptr(win), ptr(cost), None) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_last_rescore_ms(None) == -1.0
    p, ld, n_cost = C.c_void_p(), C.c_int64(0), C.c_int32(0)
    assert L.fx_device_costmap_view(None, 0, C.byref(p), C.byref(ld), C.byref(n_cost)) == _abi.FX_ERR_INVALID_ARGUMENT
    # the regime hook answers the rule, and a forced regime until it is cleared
    assert (L.fx_rescore_regime(630, 63), L.fx_rescore_regime(630, 64)) == (rp.LANE, rp.VECTOR)
    L.fx_rescore_set_regime(rp.LANE)
    assert L.fx_rescore_regime(50_388, 256) == rp.LANE
    L.fx_rescore_set_regime(0)
    assert L.fx_rescore_regime(50_388, 256) == rp.VECTOR


def test_dicts_become_rows_in_cost_names_order():
    a = dict(velocity_offset=1.0, prediction=0.2, lateral_jerk=0.3, longitudinal_jerk=-0.4, distance_to_reference_path=5.0)
    b = dict(a, jerk=0.0, lateral_jerk=7.0)                        # (a zero entry is a term upstream does not register)
    w = rescore_weights([a, b], NAMES)
    assert w.dtype == np.float64 and w.flags["C_CONTIGUOUS"] and w.shape == (2, 5)
    assert w.tolist() == [[5.0, 0.3, -0.4, 0.2, 1.0], [5.0, 7.0, -0.4, 0.2, 1.0]]
    assert rescore_weights(a, NAMES).tolist() == [[5.0, 0.3, -0.4, 0.2, 1.0]]      # one dict is one set
    assert rescore_weights((a,), NAMES).shape == (1, 5)


def test_arrays_pass_in_shape():
    w = rescore_weights([[1, 2, 3, 4, 5], [5, 4, 3, 2, -1]], NAMES)
    assert w.shape == (2, 5) and w.dtype == np.float64
    assert rescore_weights(np.arange(1.0, 6.0), NAMES).shape == (1, 5)              # one vector
    f32 = np.full((3, 5), 0.5, np.float32)[:, ::-1]
    w = rescore_weights(f32, NAMES)
    assert w.dtype == np.float64 and w.flags["C_CONTIGUOUS"] and np.all(w == 0.5)
    assert rescore_weights(np.ones((4, 7)), None).shape == (4, 7)                   # no step to hold it to: the library decides


@pytest.mark.parametrize("bad", [
    [],                                                     # no vector
    np.zeros((0, 5)),
    np.ones((2, 4)), np.ones((2, 6)), np.ones((2, 5, 1)),   # not [W][n_cost]
    [[1, 2, 3, 4, 0.0]], [[1, 2, 3, 4, -0.0]],              # a zero weight is another cost list
    [[1, 2, 3, 4, np.nan]], [[1, 2, np.inf, 4, 5]], [[-np.inf, 2, 3, 4, 5]],
    [dict(zip(NAMES[:-1], [1.0] * 4))],                     # a term of the step is missing
    [dict(zip(NAMES, [1.0] * 5), jerk=0.1)],                # a term the step has not
    [dict(zip(NAMES, [1.0, 1.0, 1.0, 0.0, 1.0]))],          # ... a zero weight says the same
    [dict(zip(NAMES, [1.0, 1.0, 1.0, np.nan, 1.0]))],
    [dict(zip(NAMES, [1.0] * 5)), [1.0] * 5],               # dicts and rows mixed
    "weights",
])
def test_value_errors(bad):
    with pytest.raises(ValueError):
        rescore_weights(bad, NAMES)


def test_dicts_need_a_step():
    with pytest.raises(ValueError, match="plan step"):
        rescore_weights([dict(zip(NAMES, [1.0] * 5))], None)


def test_planner_without_a_step():
    from frenetix_motion_planner_amd.reactive_planner import ReactivePlannerHip
    assert "device selection only" in ReactivePlannerHip.rescore.__doc__ and "occlusion walk" in ReactivePlannerHip.rescore.__doc__
    p = ReactivePlannerHip.__new__(ReactivePlannerHip)
    p.last_step = None
    with pytest.raises(ValueError, match="no plan step"):
        p.rescore([{}])


def test_committed_resource_lines():
    """profiles/rescore/: every kernel of the parent with the line it had, the new kernels without scratch or spills"""
    rows = {}
    for which in ("parent", "commit"):
        with open(os.path.join(ROOT, "profiles", "rescore", f"kernel_resources_{which}.txt")) as f:
            rows[which] = dict(line.split(None, 1) for line in f if line.strip())
    assert len(rows["parent"]) > 150 and all(rows["commit"].get(k) == v for k, v in rows["parent"].items())
    new = {k: v for k, v in rows["commit"].items() if k not in rows["parent"]}
    assert len(new) == 4 and all("rescore" in k for k in new)
    for k, v in new.items():
        f = dict(zip(v.split()[0::2], (int(x) for x in v.split()[1::2])))
        assert f["scratch"] == 0 and f["spillV"] == 0 and f["spillS"] == 0 and f["occ"] == 8 and f["VGPR"] <= 64, (k, v)


def test_reference_and_planes_on_the_host():
    """tests/rescore_planes.py: the reference is the plain statement, and the planes are what their names say"""
    assert rp.contraction_is_off()
    rng = np.random.default_rng(3)
    raw, flags = rng.normal(size=(5, 40)), np.full(40, rp.OK, np.uint32)
    flags[::7] = rp.SEL                                            # (no cost)
    w = np.array([0.5, -2.0, 3.0, 0.25, 1.5])
    for deferred in (False, True):
        got = rp.totals_of(raw, flags, w, 3, deferred)
        for c in range(40):
            s, tail = -0.0, 0.0
            for m in range(5):
                t = float(w[m]) * float(raw[m, c])
                if deferred and m > 3:
                    tail += t
                else:
                    s += t
            if deferred:
                s += tail
            want = 0.0 + s if flags[c] & rp.COSTED else np.nan
            assert int(dp.bits(got[c])) == int(dp.bits(want)) or (np.isnan(got[c]) and np.isnan(want))
    # -0.0 survives where the step's sum keeps it apart from +0.0: the rule starts at -0.0 and closes with 0.0 +
    z = rp.totals_of(np.zeros((5, 1)), np.array([rp.OK], np.uint32), np.ones(5), 3, False)
    assert int(dp.bits(z[0])) == int(dp.bits(0.0))
    assert rp.winner_of(np.array([np.nan, 2.0, 2.0, 1.0]), np.array([rp.OK, rp.OK, rp.OK, rp.SEL | rp.COL | rp.COSTED], np.uint32)) == (1, 2.0)
    assert rp.winner_of(np.array([np.nan, np.inf]), np.full(2, rp.OK, np.uint32)) == (1, np.inf)
    assert rp.winner_of(np.array([1.0]), np.array([rp.COSTED], np.uint32)) == (-1, np.inf)
    for n in rp.SIZES:
        for name in rp.PLANES:
            raw, flags = rp.plane(name, n, 5)
            r2, f2 = rp.plane(name, n, 5)
            assert raw.shape == (5, n) and flags.shape == (n,) and np.array_equal(dp.bits(raw), dp.bits(r2)) and np.array_equal(flags, f2)
        for n_vec in rp.N_VECS:
            W = rp.weight_vectors(n_vec, 5)
            assert W.shape == (n_vec, 5) and np.all(W[0] == 1.0) and (W < 0).any() == (n_vec > 1)
        win, cost, tot = rp.expected(*rp.plane("nothing_eligible", n, 5), rp.weight_vectors(3, 5), 3, False)
        assert np.all(win == -1) and np.all(cost == np.inf)
        win, _, tot = rp.expected(*rp.plane("ties_under_some", n, 5), rp.weight_vectors(3, 5), 3, False)
        assert n == 1 or (win[0] == n // 3 and win[1] == n - 1 and tot[0][n // 3] == tot[0][n - 1])
        win, _, _ = rp.expected(*rp.plane("all_equal", n, 5), rp.weight_vectors(65, 5), 3, True)
        assert np.all(win == n // 3)
