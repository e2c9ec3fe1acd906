"""The NumPy restatement of the collision probability as the prediction cost (tests/predprob_restatement.py) against the
reference's own get_collision_probability_fast and the summation of prediction_costs (tests/golden/gen_predprob_golden.py):
predprob_obs5.npz, predprob_mixed_obs6.npz and predprob_config3_obs20.npz on the trajectories and predictions of the risk
goldens.  1e-12 (1 + |want|) per step, per obstacle and per candidate; the quirks of the upstream function one by one."""
import os

import numpy as np
import pytest

from tests import predprob_restatement as pp
from tests.test_risk_golden import _load

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PASS_GATE = {"obs5": (9, 90), "mixed_obs6": (17, 85), "config3_obs20": (82, 82)}   # candidates that pass the 5 m gate somewhere
POSITIVE = {"obs5": 5, "mixed_obs6": 15, "config3_obs20": 82}   # ... whose stored sum is positive (gen_predprob_golden.py: the shim's noise)
EGO_L, EGO_W = 4.508, 1.61


def _golden(name):
    g, preds, _, _ = _load("risk_" + name)
    return g, preds, np.load(os.path.join(GOLDEN, "predprob_" + name + ".npz"))


@pytest.mark.parametrize("name", list(PASS_GATE))
def test_restatement_matches_reference_golden(name):
    g, preds, want = _golden(name)
    P = g["planes"]
    assert np.array_equal(g["plane_ids"], want["plane_ids"])
    prob, prob_obs, steps = pp.prediction_probability(P[:, 0], P[:, 1], P[:, 2], preds, *want["ego"])
    for got, ref in ((steps, want["steps"]), (prob_obs, want["prob_obs"]), (prob, want["prob"])):
        assert got.shape == ref.shape
        assert np.all(np.abs(got - ref) <= 1e-12 * (1 + np.abs(ref))), np.abs(got - ref).max()


@pytest.mark.parametrize("name", list(PASS_GATE))
def test_goldens_are_not_trivial(name):
    """as many candidates as the generator found pass the gate somewhere, none within 1e-6 m of it; the sums they stand for are
    there (the restatement's are positive for every one of them, the reference's for those above its shim's noise: see
    gen_predprob_golden.py)"""
    g, preds, want = _golden(name)
    P = g["planes"]
    passes = np.zeros(len(P), bool)
    for pr in preds.values():
        passes |= np.any(~(pp.gate_distances(P[:, 0], P[:, 1], pr) > 5.0), axis=1)
    assert (int(passes.sum()), len(P)) == PASS_GATE[name] and int(want["n_pass_gate"]) == PASS_GATE[name][0]
    assert not pp.near_gate(P[:, 0], P[:, 1], preds).any()
    prob, _, _ = pp.prediction_probability(P[:, 0], P[:, 1], P[:, 2], preds, *want["ego"])
    assert np.array_equal(prob > 0, passes)
    assert np.all(want["prob"][~passes] == 0) and int((want["prob"] > 0).sum()) == POSITIVE[name]
    assert np.all(np.abs(want["prob"][~(want["prob"] > 0)]) <= 1e-15)   # (what is not positive is the shim's cancellation noise)


def _traj(n=31):
    t = np.arange(n) * 0.1
    return (10.0 * t)[None, :], np.zeros((1, n)), np.zeros((1, n))


def _pred(n, cov=None, dy=1.0):
    t = np.arange(n) * 0.1
    c = np.tile(np.array([[0.4, 0.1], [0.1, 0.3]]) if cov is None else np.asarray(cov, float), (n, 1, 1))
    return dict(pos_list=np.stack([10.0 * t + 1.0, np.full(n, dy)], axis=1), cov_list=c, orientation_list=np.zeros(n),
                shape=dict(length=4.5, width=1.8))


def test_no_obstacles_is_zero():
    x, y, th = _traj()
    prob, prob_obs, steps = pp.prediction_probability(x, y, th, {}, EGO_L, EGO_W)
    assert prob.shape == (1,) and prob[0] == 0.0 and prob_obs.shape == (1, 0) and steps.shape == (1, 0, 30)


def test_short_prediction_as_upstream():
    """ego point i pairs with prediction i - 1 and needs i < len(pos_list): a prediction of n entries fills steps 1 .. n - 1 and
    its LAST entry is never used; the probabilities of the steps it covers are those of the long prediction"""
    x, y, th = _traj()
    long_, short = _pred(31), _pred(12)
    a = pp.step_probabilities(x, y, th, long_, EGO_L, EGO_W)
    b = pp.step_probabilities(x, y, th, short, EGO_L, EGO_W)
    assert a.shape == b.shape == (1, 30)
    assert np.array_equal(b[:, :11], a[:, :11]) and np.all(b[:, 11:] == 0) and np.all(a[:, :11] > 0) and a[0, 11] > 0
    changed = _pred(12)
    changed["pos_list"][-1] += 100.0
    changed["cov_list"][-1] *= 7.0
    assert np.array_equal(pp.step_probabilities(x, y, th, changed, EGO_L, EGO_W), b)
    # an empty and a one-entry prediction give nothing
    for n in (0, 1):
        assert np.all(pp.step_probabilities(x, y, th, _pred(n), EGO_L, EGO_W) == 0)


def test_zero_covariance_becomes_a_tenth_of_identity():
    x, y, th = _traj()
    zero, tenth = _pred(31, cov=np.zeros((2, 2))), _pred(31, cov=0.1 * np.eye(2))
    a = pp.step_probabilities(x, y, th, zero, EGO_L, EGO_W)
    assert np.array_equal(a, pp.step_probabilities(x, y, th, tenth, EGO_L, EGO_W)) and np.all(a > 0)
    # only an ALL-zero matrix is replaced
    part = _pred(31, cov=np.array([[0.1, 0.0], [0.0, 0.2]]))
    assert not np.array_equal(a, pp.step_probabilities(x, y, th, part, EGO_L, EGO_W))


def test_gate_is_taken_over_three_means():
    """an obstacle whose centre is 6 m ahead but whose rear (length 4.5) is within 5 m passes the gate"""
    x, y, th = _traj()
    pr = _pred(31, dy=0.0)
    pr["pos_list"][:, 0] += 5.0                       # centre 6 m ahead of ego point i - 1 ... 5 m ahead of ego point i
    d = pp.gate_distances(x, y, pr)
    assert np.all(d < 5.0) and np.all(np.hypot(pr["pos_list"][:-1, 0] - x[0, 1:], pr["pos_list"][:-1, 1]) >= 5.0 - 1e-9)
    assert np.all(pp.step_probabilities(x, y, th, pr, EGO_L, EGO_W) > 0)
    pr["shape"]["length"] = 0.0                       # without the length the same centres are outside
    pr["pos_list"][:, 0] += 0.5
    assert np.all(pp.step_probabilities(x, y, th, pr, EGO_L, EGO_W) == 0)


def test_sum_order_and_resum():
    rng = np.random.default_rng(0)
    raw = rng.uniform(0, 3, (50, 5))
    w = np.array([5.0, 0.2, 0.2, 0.2, 1.0])
    prob = rng.uniform(0, 1, 50)
    want = np.zeros(50)
    for c in range(50):
        s = -0.0
        for m in range(5):
            s += w[m] * (prob[c] if m == 3 else raw[c, m])
        want[c] = 0.0 + s
    assert np.array_equal(pp.resum(raw, w, 3, prob), want)
    assert np.array_equal(pp.resum(raw, w, 3, prob, deferred=True), want)   # one term behind the prediction: the same additions
    flags = np.full(50, 0x3B, np.uint32)
    flags[::2] |= 0x4
    want[1] = np.nan
    assert pp.best_index(want, flags) == int(np.arange(50)[1::2][1:][np.argmin(want[1::2][1:])])
    assert pp.best_index(want, np.zeros(50, np.uint32)) == -1
