"""What fx_eval_hypotheses_batch refuses: every refusal names the agent, leaves the caller's outputs untouched,
the steps' flag and cost planes and fx_device_bytes as they were, fx_last_hypotheses_info reporting what it reported before, and a
following good call correct."""
import ctypes as C

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi
from tests import device_planes as dp
from tests import hypotheses_scene as hs
from tests.test_hypotheses_batch_gpu import KW, same, scene

pytestmark = pytest.mark.gpu

SENTINEL = -77


def raw_call(e, agents, n_hyp, hyps, *, n_agents=None, have=("n_hyp", "hyp", "out", "winner", "cost"), null_field=None):
    """fx_eval_hypotheses_batch as a C caller has it; hyps: the hypotheses one behind the other; null_field: (position, array) that
    is NULL.  Returns (status, winner, cost) -- the outputs pre-filled with a sentinel"""
    from frenetix_motion_planner_amd._lib import lib
    H = max(len(hyps), 1)
    arr = (_abi.FxHypothesis * H)()
    keep = []
    for h, hyp in enumerate(hyps):
        for name, key, typ in (("obs_pos", "pos", np.float64), ("obs_cov_inv", "cov_inv", np.float64), ("obs_npred", "npred", np.int32),
                               ("obs_hull", "hull", np.float64), ("obs_nhull", "nhull", np.int32)):
            a = np.ascontiguousarray(hyp[key], dtype=typ)
            keep.append(a)
            setattr(arr[h], name, None if null_field == (h, name) else a.ctypes.data)
    total = max(int(sum(max(n, 0) for n in n_hyp)), H)
    win, cost = np.full(total, SENTINEL, np.int64), np.full(total, float(SENTINEL))
    o = _abi.FxHypothesisOutputs()
    o.winner, o.cost = (win.ctypes.data if "winner" in have else None), (cost.ctypes.data if "cost" in have else None)
    ids = None if agents is None else np.array(agents, np.int32)
    nh = np.array(n_hyp, np.int32)
    rc = lib().fx_eval_hypotheses_batch(e._ctx, len(n_hyp) if n_agents is None else n_agents,
                                        None if ids is None else ids.ctypes.data_as(C.c_void_p),
                                        nh.ctypes.data_as(C.c_void_p) if "n_hyp" in have else None, arr if "hyp" in have else None,
                                        C.byref(o) if "out" in have else None)
    return rc, win, cost


def state(e, n_agents):
    """what a refusal must leave alone: every agent's costs, flags and cost map"""
    parts = []
    for a in range(n_agents):
        cost, flags = e.costs(a)
        parts += [dp.bits(cost), flags, dp.bits(e.costmap(a))]
    return parts


def unchanged(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals_before_a_finished_step():
    inps = [scene(130, 4), scene(65, 7)]
    own = [hs.hypothesis_arrays(i.obstacles, i.obstacles["K"], i.obstacles["P"]) for i in inps]
    assert raw_call(type("E", (), {"_ctx": None}), None, [1, 1], own)[0] == _abi.FX_ERR_INVALID_ARGUMENT     # no context
    assert raw_call(type("E", (), {"_ctx": None}), None, [], [], n_agents=-1)[0] == _abi.FX_ERR_INVALID_ARGUMENT
    with hs.engine(max_candidates=sum(i.n_candidates for i in inps) + 128, max_agents=2) as e:
        b0 = e.device_bytes
        rc, win, cost = raw_call(e, None, [1, 1], own)
        assert rc == _abi.FX_ERR_NOT_READY and e.device_bytes == b0 and np.all(win == SENTINEL) and np.all(cost == SENTINEL)
        assert raw_call(e, None, [], [], n_agents=0)[0] == _abi.FX_OK and e.device_bytes == b0              # the documented no-op
        e.set_obstacle_stage(2, 3)
        results = e.plan_batch(inps)
        got = e.hypotheses_batch([[own[0]], [own[1]]])
        assert [int(g["winner"][0]) for g in got] == [r["best_index"] for r in results]


def test_refusals_leave_everything_as_it_was():
    from frenetix_motion_planner_amd._lib import lib
    inps = [scene(130, 4), scene(65, 7), scene(257, 2), scene(64, 0)]
    assert inps[3].obstacles["K"] == 0
    own = [hs.hypothesis_arrays(i.obstacles, i.obstacles["K"], i.obstacles["P"]) for i in inps[:3]]
    with hs.engine(max_candidates=sum(i.n_candidates for i in inps) + 64 * 4, max_agents=4) as e:
        e.set_obstacle_stage(2, 3)
        results = e.plan_batch(inps)
        sets = [[own[0]] * 2, [own[1]], [own[2]] * 3]
        flat = [h for s in sets for h in s]
        good = e.hypotheses_batch(sets, agents=[0, 1, 2], **KW)
        assert [int(g["winner"][0]) for g in good] == [r["best_index"] for r in results[:3]]
        info = e.last_hypotheses_info
        assert info == dict(steps_per_item=3, rounds=1, launches=3)
        before, b0 = state(e, 4), e.device_bytes
        R, CAP = _abi.FX_ERR_INVALID_ARGUMENT, _abi.FX_ERR_CAPACITY

        def refused(code, *args, **kw):
            rc, win, cost = raw_call(e, *args, **kw)
            assert rc == code, (rc, code, args[:2], kw)
            assert np.all(win == SENTINEL) and np.all(cost == SENTINEL), (args[:2], kw)                      # the outputs untouched
            assert e.last_hypotheses_info == info and e.device_bytes == b0 and unchanged(before, state(e, 4)), (args[:2], kw)
            after = e.hypotheses_batch(sets, agents=[0, 1, 2], **KW)                                         # a good call behind it
            for g, w in zip(after, good):
                same(g, w, ("behind a refusal", args[:2], kw))

        refused(R, [0, 1, 2], [2, 1, 3], flat, n_agents=-1)
        for missing in ("n_hyp", "hyp", "out", "winner", "cost"):
            refused(R, [0, 1, 2], [2, 1, 3], flat, have=tuple(x for x in ("n_hyp", "hyp", "out", "winner", "cost") if x != missing))
        refused(R, [0, 1, 4], [2, 1, 3], flat)                          # out of range
        refused(R, [0, -1, 2], [2, 1, 3], flat)
        refused(R, [0, 1, 0], [2, 1, 3], [own[0]] * 2 + [own[1]] + [own[0]] * 3)   # listed twice
        refused(R, [0, 1, 2], [2, 0, 3], [own[0]] * 2 + [own[2]] * 3)   # no hypothesis for one agent
        refused(R, [0, 1, 2], [2, -1, 3], [own[0]] * 2 + [own[2]] * 3)
        refused(R, [0, 3], [2, 1], [own[0]] * 3)                        # an agent uploaded without obstacles
        for field in ("obs_pos", "obs_cov_inv", "obs_npred", "obs_hull", "obs_nhull"):
            refused(R, [0, 1, 2], [2, 1, 3], flat, null_field=(3, field))        # a NULL array in agent 2's first hypothesis
        M = _abi.FX_HYPOTHESES_MAX
        refused(CAP, [1, 0], [1, M + 1], [own[1]] + [own[0]] * (M + 1))
        # the wrapper states them by name
        with pytest.raises(ValueError, match="agent 1: fx_eval_hypotheses_batch: n_hyp 0"):
            e.hypotheses_batch([[own[0]], [], [own[2]]])
        with pytest.raises(ValueError, match="agent 3: agent 3 was uploaded without obstacles"):
            e.hypotheses_batch([[own[0]], [own[0]]], agents=[0, 3])
        with pytest.raises(ValueError, match="agent 2 listed twice"):
            e.hypotheses_batch([[own[2]], [own[2]]], agents=[2, 2])
        with pytest.raises(ValueError, match="agent 7 out of range"):
            e.hypotheses_batch([[own[0]], [own[0]]], agents=[0, 7])
        with pytest.raises(ValueError, match=f"agent 0: {M + 1} hypotheses: at most {M} per call"):
            e.hypotheses_batch([[own[1]], [own[0]] * (M + 1)], agents=[1, 0])
        with pytest.raises(ValueError, match="obstacles in a hypothesis"):
            e.hypotheses_batch([[own[0]], [own[1]]], agents=[1, 0])     # more obstacles than agent 0's upload
        with pytest.raises(ValueError, match="2 lists of prediction sets for 3 agents"):
            e.hypotheses_batch([[own[0]], [own[1]]], agents=[0, 1, 2])
        assert e.last_hypotheses_info == info and e.device_bytes == b0 and unchanged(before, state(e, 4))
        # the inputs rewritten since the step
        e.update_state(e.make_state_update(v_des=inps[1].v_des + 1.0), 1)
        rc, win, cost = raw_call(e, [0, 1, 2], [2, 1, 3], flat)
        assert rc == _abi.FX_ERR_NOT_READY and np.all(win == SENTINEL) and e.device_bytes == b0
        with pytest.raises(ValueError, match="rewritten"):
            e.hypotheses_batch(sets, agents=[0, 1, 2])
        e.update_state(e.make_state_update(v_des=inps[1].v_des), 1)
        e.evaluate()
        e.finish()
        assert unchanged(before, state(e, 4))
        for g, w in zip(e.hypotheses_batch(sets, agents=[0, 1, 2], **KW), good):
            same(g, w, "behind the step run again")
        # the block is grow-only and shared with the per-agent call: neither call moves it once it has its size
        e.hypotheses(sets[2], agent=2, **KW)
        assert e.device_bytes == b0
        lib().fx_hypotheses_set_scratch_limit(0)
