"""The hypotheses pass of a whole agent batch without a GPU: the entry point is exported and declared and the
ABI version stays (additive); what the library refuses without a device and the documented no-op; the docstrings say what the calls
are; AgentBatchHip.what_if refuses unknown and stale agents by name and issues one engine call per context, on a stand-in engine;
the committed resource lines hold every kernel of the parent with the line it had and the new kernels without scratch."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc")


def test_the_entry_point_is_exported_and_declared():
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    sym = "fx_eval_hypotheses_batch"
    assert hasattr(L, sym) and re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.exported_symbols()
    assert L.fx_abi_version() == _abi.FX_ABI_VERSION == 15      # additive: the version stays
    assert int(re.search(r"#define FX_ABI_VERSION (\d+)", hdr).group(1)) == 15
    assert L.fx_eval_hypotheses_batch.argtypes == _abi.FX_EVAL_HYPOTHESES_BATCH_ARGS and len(_abi.FX_EVAL_HYPOTHESES_BATCH_ARGS) == 6
    # one launcher, declared once and named once; the stubs follow from the list
    launch = open(os.path.join(CSRC, "fx_launch.h")).read()
    assert launch.count("fx_launch_hypotheses_batch") == 2 and "X(fx_launch_hypotheses_batch)" in launch
    assert "fx_launch_hypotheses_batch" not in open(os.path.join(CSRC, "fx_host_stubs.cpp")).read()
    assert not os.path.exists(os.path.join(CSRC, "fx_api_hypotheses_batch.hip"))
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "fx_hypotheses_batch_plan.h" in mk and "fx_hypotheses_batch_kernel.h" in mk


def test_refusals_that_need_no_device():
    L = _lib.lib()
    hyp, out = (_abi.FxHypothesis * 1)(), _abi.FxHypothesisOutputs()
    win, cost = np.full(1, -77, np.int64), np.full(1, -77.0)
    out.winner, out.cost = win.ctypes.data, cost.ctypes.data
    n_hyp = np.ones(1, np.int32)
    p = n_hyp.ctypes.data_as(C.c_void_p)
    assert L.fx_eval_hypotheses_batch(None, 1, None, p, hyp, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT      # NULL context
    assert b"context is NULL" in L.fx_last_error()
    assert L.fx_eval_hypotheses_batch(None, -1, None, p, hyp, C.byref(out)) == _abi.FX_ERR_INVALID_ARGUMENT
    assert b"n_agents -1" in L.fx_last_error()
    # the documented no-op: no agent, nothing touched -- whatever else is passed
    assert L.fx_eval_hypotheses_batch(None, 0, None, None, None, None) == _abi.FX_OK
    assert L.fx_eval_hypotheses_batch(None, 0, None, p, hyp, C.byref(out)) == _abi.FX_OK
    assert win[0] == -77 and cost[0] == -77.0


def test_docstrings():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from frenetix_motion_planner_amd.multiagent import AgentBatchHip
    doc = FrenetEngine.hypotheses_batch.__doc__
    assert "fx_eval_hypotheses_batch" in doc and "ONE call" in doc and "views" in doc and "hypothesis_arrays" in doc
    doc = AgentBatchHip.what_if.__doc__
    assert "device selection only" in doc and "ONE engine.hypotheses_batch per engine context" in doc and "refused by name" in doc


class StandInEngine:
    """counts hypotheses_batch calls and answers (agent, set index) so that the routing shows"""

    def __init__(self):
        self.calls = []

    def hypotheses_batch(self, sets, agents=None):
        self.calls.append((list(agents), [len(s) for s in sets]))
        assert all(s["K"] == 0 or s["P"] >= 1 for ss in sets for s in ss)            # packed predictions
        return [dict(winner=np.array([100 * a + h for h in range(len(s))]), cost=np.array([float(a)] * len(s)),
                     n_collisions=np.array([h for h in range(len(s))])) for a, s in zip(agents, sets)]


def stand_in_batch():
    from frenetix_motion_planner_amd.multiagent import AgentBatchHip
    e1, e2 = StandInEngine(), StandInEngine()

    def agent(aid, eng, slot, stale=False, step=True):
        last = SimpleNamespace(engine=eng, agent=slot, _stale=stale) if step else None
        return SimpleNamespace(id=aid, planner=SimpleNamespace(last_step=last, N=30))

    batch = AgentBatchHip.__new__(AgentBatchHip)
    batch.agents = [agent(11, e1, 0), agent(12, e2, 0), agent(13, e1, 1), agent(14, e2, 1, stale=True), agent(15, e1, 2, step=False)]
    return batch, e1, e2


def test_what_if_refuses_unknown_and_stale_agents_by_name():
    batch, e1, e2 = stand_in_batch()
    with pytest.raises(ValueError, match="agent 99 is not of this batch"):
        batch.what_if({11: [{}], 99: [{}]})
    with pytest.raises(ValueError, match="agent 14 has no current plan step"):
        batch.what_if({11: [{}], 14: [{}]})
    with pytest.raises(ValueError, match="agent 15 has no current plan step"):
        batch.what_if({15: [{}]})
    assert not e1.calls and not e2.calls                                  # refused before any call


def test_what_if_issues_one_call_per_context():
    batch, e1, e2 = stand_in_batch()
    out = batch.what_if({13: [{}, {}], 12: [{}], 11: [{}, {}, {}]})
    assert e1.calls == [([1, 0], [2, 3])] and e2.calls == [([0], [1])]
    assert list(out) == [13, 12, 11]
    assert out[13] == [(100, 1.0, 0), (101, 1.0, 1)] and out[12] == [(0, 0.0, 0)] and out[11] == [(0, 0.0, 0), (1, 0.0, 1), (2, 0.0, 2)]
    assert batch.what_if({}) == {} and len(e1.calls) == 1


def test_committed_resource_lines():
    """profiles/hypotheses_batch/: every kernel of the parent with the line it had, the parent's list the previous pull request's
    list of this commit, the five new kernels without scratch or spills; and the instruction text of every kernel of the parent is
    what it was (tools/isa/compare_isa.py's list): zero functions changed, the new ones only in the commit"""
    rows = {}
    for which in ("parent", "commit"):
        with open(os.path.join(ROOT, "profiles", "hypotheses_batch", f"kernel_resources_{which}.txt")) as f:
            rows[which] = dict(line.split(None, 1) for line in f if line.strip())
    assert len(rows["parent"]) > 190 and all(rows["commit"].get(k) == v for k, v in rows["parent"].items())
    with open(os.path.join(ROOT, "profiles", "launchers", "kernel_resources_commit.txt")) as f:
        prev = dict(line.split(None, 1) for line in f if line.strip())
    assert prev == rows["parent"]
    new = {k: v for k, v in rows["commit"].items() if k not in rows["parent"]}
    assert len(new) == 5 and all("fxhy" in k and "fx_hyp_batch_" in k for k in new)
    fields = lambda v: dict(zip(v.split()[0::2], (int(x) for x in v.split()[1::2])))
    for k, v in new.items():
        f = fields(v)
        assert f["scratch"] == 0 and f["spillV"] == 0 and f["spillS"] == 0 and f["occ"] >= 4 and f["VGPR"] <= 128, (k, v)
    # the item kernels keep the per-agent kernels' vector registers: 58 / 64 / 76 for 2 / 3 / 5 steps per item
    for ch, vgpr in ((2, 58), (3, 64), (5, 76)):
        one = fields(rows["commit"][f"_ZN4fxhy18fx_hyp_item_kernelILi{ch}EEEv9FxHypArgs"])
        bat = fields(next(v for k, v in new.items() if f"fx_hyp_batch_item_kernelILi{ch}E" in k))
        assert one["VGPR"] == vgpr and bat["VGPR"] <= vgpr and bat["lds"] == 0
    with open(os.path.join(ROOT, "profiles", "hypotheses_batch", "isa_compared.txt")) as f:
        isa = [l.split() for l in f if l.strip() and not l[0].isdigit()]
    same = {l[1] for l in isa if l[0] == "identical"}
    assert same == set(rows["parent"])
    assert not [l for l in isa if l[0] == "differs"] and {l[-1] for l in isa if l[0] != "identical"} == set(new)
    assert all(l[:3] == ["only", "in", "B"] for l in isa if l[0] != "identical")
