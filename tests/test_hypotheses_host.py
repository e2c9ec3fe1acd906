"""The hypotheses pass without a GPU: the entry points are exported and declared and the ABI version stays
(additive, as sections 15 to 24 were); the ctypes structs have the sizes of the header's; what the library refuses without a device;
`problem.hypothesis_arrays` pads with absent obstacles, re-strides and refuses more obstacles than the upload has; the committed
resource lines hold every kernel of the parent with the line it had and the new kernels without scratch; and the NumPy selection the
GPU tests compare with (tests/hypotheses_scene.py) holds what it claims on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, _lib
from frenetix_motion_planner_amd.problem import hypothesis_arrays, pack_predictions
from tests import hypotheses_scene as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_exported_and_declared():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    for sym in ("fx_eval_hypotheses_agent", "fx_last_hypotheses_ms", "fx_last_hypotheses_info"):
        assert hasattr(L, sym) and re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.exported_symbols()
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays
    assert int(re.search(r"#define FX_HYPOTHESES_MAX (\d+)", hdr).group(1)) == _abi.FX_HYPOTHESES_MAX >= 1024


def test_struct_sizes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    for name, cls in (("FxHypothesis", _abi.FxHypothesis), ("FxHypothesisOutputs", _abi.FxHypothesisOutputs)):
        body = re.search(rf"typedef struct {name} \{{(.*?)\}} {name};", hdr, re.S).group(1)
        fields = re.findall(r"\*\s*(\w+)\s*;", body)
        assert fields == [f for f, _ in cls._fields_]                       # the same pointers in the same order
        assert C.sizeof(cls) == 8 * len(fields) and all(t is C.c_void_p for _, t in cls._fields_)
    assert C.sizeof(_abi.FxHypothesis) == 40 and C.sizeof(_abi.FxHypothesisOutputs) == 48


def test_refusals_that_need_no_device():
    L = _lib.lib()
    hyp, out = (_abi.FxHypothesis * 1)(), _abi.FxHypothesisOutputs()
    assert L.fx_eval_hypotheses_agent(None, 0, 1, hyp, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert L.fx_last_hypotheses_ms(None) == -1.0
    assert L.fx_last_hypotheses_info(None, None, None, None) == _abi.FX_ERR_INVALID_ARGUMENT


def scene_packed(n_obstacles=3):
    inp = hs.make(hs.GRIDS["small"], n_obstacles, hull_builder=None)
    return pack_predictions(inp.predictions, hs.N + 1, hs.hull_builder()), inp


def test_hypothesis_arrays_pads_and_restrides():
    packed, _ = scene_packed(3)
    K0, P0 = packed["K"], packed["P"]
    assert K0 == 3 and P0 == hs.N and packed["nhull"].min() > 0
    same = hypothesis_arrays(packed, K0, P0)
    for k in ("pos", "cov_inv", "npred", "hull", "nhull"):
        assert np.array_equal(same[k], np.asarray(packed[k]).reshape(same[k].shape)) and same[k].flags["C_CONTIGUOUS"]
    assert same["npred"].dtype == np.int32 and same["nhull"].dtype == np.int32
    # padded with absent obstacles up to the upload's K
    wide = hypothesis_arrays(packed, 7, P0)
    assert wide["pos"].shape == (7, P0, 2) and wide["cov_inv"].shape == (7, P0, 4) and wide["hull"].shape == (7, P0 - 1, 6)
    assert np.array_equal(wide["pos"][:3], same["pos"]) and np.array_equal(wide["hull"][:3], same["hull"])
    assert not wide["npred"][3:].any() and not wide["nhull"][3:].any() and not wide["pos"][3:].any()
    assert np.array_equal(wide["npred"][:3], packed["npred"]) and np.array_equal(wide["nhull"][:3], packed["nhull"])
    # re-strided to a longer and to a shorter P
    long = hypothesis_arrays(packed, 3, P0 + 5)
    assert long["pos"].shape == (3, P0 + 5, 2) and np.array_equal(long["pos"][:, :P0], same["pos"]) and not long["pos"][:, P0:].any()
    assert np.array_equal(long["hull"][:, :P0 - 1], same["hull"]) and np.array_equal(long["nhull"], same["nhull"])
    short = hypothesis_arrays(packed, 3, 10)
    assert short["pos"].shape == (3, 10, 2) and np.array_equal(short["pos"], same["pos"][:, :10])
    assert np.array_equal(short["cov_inv"], same["cov_inv"][:, :10]) and np.array_equal(short["hull"], same["hull"][:, :9])
    assert np.all(short["nhull"] == 9) and np.array_equal(short["npred"], same["npred"])
    # no obstacle at all: every one absent
    none = hypothesis_arrays(pack_predictions({}, hs.N + 1, hs.hull_builder()), 4, 12)
    assert none["K"] == 4 and none["P"] == 12 and not none["npred"].any() and not none["nhull"].any() and none["hull"].shape == (4, 11, 6)


def test_hypothesis_arrays_value_errors():
    packed, _ = scene_packed(3)
    with pytest.raises(ValueError, match="3 predicted obstacles in a hypothesis for an upload of K=2"):
        hypothesis_arrays(packed, 2, packed["P"])
    for K, P in ((0, 10), (3, 1), (-1, 10)):
        with pytest.raises(ValueError):
            hypothesis_arrays(packed, K, P)


def test_planner_without_a_step():
    from frenetix_motion_planner_amd.reactive_planner import ReactivePlannerHip
    assert "device selection only" in ReactivePlannerHip.what_if.__doc__ and "occlusion walk" in ReactivePlannerHip.what_if.__doc__
    p = ReactivePlannerHip.__new__(ReactivePlannerHip)
    p.last_step = None
    with pytest.raises(ValueError, match="no plan step"):
        p.what_if([{}])


def test_committed_resource_lines():
    """profiles/hypotheses/: every kernel of the parent with the line it had, the five new kernels without scratch or spills; and
    the instruction text of every kernel of the parent is what it was (tools/isa/compare_isa.py's list)"""
    rows = {}
    for which in ("parent", "commit"):
        with open(os.path.join(ROOT, "profiles", "hypotheses", f"kernel_resources_{which}.txt")) as f:
            rows[which] = dict(line.split(None, 1) for line in f if line.strip())
    assert len(rows["parent"]) > 180 and all(rows["commit"].get(k) == v for k, v in rows["parent"].items())
    # the parent's list is the previous pull request's list of this commit's kernels
    with open(os.path.join(ROOT, "profiles", "rescore_batch", "kernel_resources_commit.txt")) as f:
        prev = dict(line.split(None, 1) for line in f if line.strip())
    assert prev == rows["parent"]
    new = {k: v for k, v in rows["commit"].items() if k not in rows["parent"]}
    assert len(new) == 5 and all("fxhy" in k for k in new)
    for k, v in new.items():
        f = dict(zip(v.split()[0::2], (int(x) for x in v.split()[1::2])))
        assert f["scratch"] == 0 and f["spillV"] == 0 and f["spillS"] == 0 and f["occ"] >= 4 and f["VGPR"] <= 128, (k, v)
    with open(os.path.join(ROOT, "profiles", "hypotheses", "isa_compared.txt")) as f:
        isa = [l.split() for l in f if l.strip() and not l[0].isdigit()]
    same = {l[1] for l in isa if l[0] == "identical"}
    assert same == set(rows["parent"]) and {l[-1] for l in isa if l[0] != "identical"} == set(new)


def test_the_numpy_selection_on_the_host():
    OK = hs.SEL | hs.COSTED
    f = np.array([OK, OK, OK, OK | hs.BND, hs.COSTED, OK], np.uint32)
    tot = np.array([3.0, 1.0, 1.0, 0.5, 0.1, np.nan])
    col = np.array([False, True, False, False, False, False])
    assert hs.numpy_selection(tot, col, f) == (2, 1.0, 1)                    # the colliding tie at the lower index orders before
    assert hs.numpy_selection(tot, np.array([True, False, True, False, False, False]), f) == (1, 1.0, 0)
    assert hs.numpy_selection(tot, np.array([True, True, True, True, True, True]), f) == (-1, np.inf, 5)   # all selectable collide
    assert hs.numpy_selection(np.full(6, np.nan), col, f) == (-1, np.inf, 1)
