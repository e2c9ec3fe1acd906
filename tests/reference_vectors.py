"""An engine's plan step against the reference planner's stored vectors (tests/golden/*.npz) DIRECTLY -- every expectation is
read from the fixture; the CPU oracle contributes only which candidates the reference decides by the last ulp (`margin`,
`frag_sites`), what else those may legitimately be (oracle.admissible_outcomes) and the conditioning of the reference's own
arithmetic (tests/admissible.py).  Engine-agnostic: anything with FrenetEngine's read-back surface (costs, costmap, coeffs,
plane, topk) -- the HIP engine in tests/test_hip_reference_vectors.py, tests/oracle_engine.OracleEngine in
tests/test_reference_vectors_cpu.py, where the comparison itself is shown to notice every kind of wrong answer.

The tolerances are the ones the suite already holds the oracle (tests/test_oracle_golden.py) and the device
(tests/test_hip_parity.py) to; none is new.  One door, the one compare() of test_hip_parity.py has: a robust candidate whose cost,
kinematic cost term or plane misses the flat bound passes at the conditioning-scaled bound only if its conditioning exceeds
WELL_CONDITIONED; such candidates are counted ("scaled") and named in the tally.
"""
import math

import numpy as np

from frenetix_motion_planner_amd import _abi
from tests.admissible import (FRAGILE_STATE_TOL, conditioning_many, kinematic_conditioning_many, matches_one_outcome,
                              path_length_weight)

STATE_TOL = 1e-9
COST_RTOL = 1e-9
COSTMAP_RTOL = 1e-8
COEFF_RTOL = 1e-10
FRAGILE = 1e-9
WELL_CONDITIONED = 1e3
KINEMATIC_COSTS = ("velocity_offset", "acceleration", "jerk", "path_length")
TOPK = 64
ALL_IDS_UP_TO = 12_000      # fixtures up to this many candidates: the coefficient rows of every candidate
MAX_STRIDE = 7


def new_tally():
    return dict(calls=0, checked=0, nonrobust=0, nonrobust_fixture=0, nonrobust_other=0, near_tie_ranks=0, scaled=0, scaled_ids=[],
                coeff_rows=0, winner_differs=0, max_cost=0.0, max_costmap=0.0, max_coeff_lon=0.0, max_coeff_lat=0.0, max_tau_lat=0.0,
                max_plane=0.0)


def add_tally(total, t):
    for k, v in t.items():
        if k.startswith("max_"):
            total[k] = max(total[k], v)
        elif isinstance(v, list):
            total[k] = total[k] + v
        else:
            total[k] += v
    return total


def format_tally(t):
    return (f"reference vectors, direct: {t['calls']} steps, {t['checked']} candidates checked, {t['coeff_rows']} coefficient rows, "
            f"{t['nonrobust']} non-robust ({t['nonrobust_fixture']} as the fixture / {t['nonrobust_other']} another admissible outcome), "
            f"{t['near_tie_ranks']} admitted near-tie ranks, {t['scaled']} scaled, max rel err cost {t['max_cost']:.2e} "
            f"costmap {t['max_costmap']:.2e} coeff_lon {t['max_coeff_lon']:.2e} coeff_lat {t['max_coeff_lat']:.2e} "
            f"tau_lat {t['max_tau_lat']:.2e} plane {t['max_plane']:.2e}")


def coeff_ids_for(fx, robust):
    """Candidates whose coefficient rows are read back (one synchronisation each): all of them up to ALL_IDS_UP_TO candidates;
    beyond, a stride of at most MAX_STRIDE coprime to nD and nV * nD (every t, v and d sample index occurs), every non-robust
    candidate and the first TOPK of the reference's walk list."""
    n = len(fx["valid"])
    if n <= ALL_IDS_UP_TO:
        return np.arange(n)
    nD = len(fx["d_order"])
    nVD = len(fx["v_order"]) * nD
    stride = max(s for s in range(1, MAX_STRIDE + 1) if math.gcd(s, nD) == 1 and math.gcd(s, nVD) == 1)
    return np.unique(np.concatenate([np.arange(0, n, stride), np.nonzero(~robust)[0], fx["walk_ids"][:TOPK].astype(np.int64)]))


def gather_planes(eng, ids, agent=0):
    """[len(ids), 14, S] planes of the candidates `ids` through the engine's per-plane read-back"""
    ids = np.asarray(ids, dtype=np.int64)
    return np.ascontiguousarray(np.stack([eng.plane(p, agent)[:, ids] for p in range(_abi.FX_NUM_PLANES)]).transpose(2, 0, 1))


def _near_tie_ranks(ref_ids, got_ids, ref_cost, what):
    """ranks at which two id lists differ; each must sit where the neighbouring REFERENCE costs are closer than the cost
    tolerance (the rule of tests/test_oracle_golden.py::test_costs_and_order).  Returns how many were admitted."""
    ref_ids, got_ids = np.asarray(ref_ids, dtype=np.int64), np.asarray(got_ids, dtype=np.int64)
    assert len(ref_ids) == len(got_ids), f"{what}: {len(got_ids)} entries against the reference's {len(ref_ids)}"
    differ = np.nonzero(ref_ids != got_ids)[0]
    if len(differ):
        gaps = np.diff(ref_cost[ref_ids])
        for j in differ:
            near = min(gaps[max(j - 1, 0)], gaps[min(j, len(gaps) - 1)])
            assert near < 1e-9 * max(1.0, abs(ref_cost[ref_ids[j]])), \
                f"{what}: rank {j} holds candidate {got_ids[j]}, the reference's {ref_ids[j]} (neighbouring reference costs {near} apart)"
    return len(differ)


def check_against_fixture(eng, inp, res, fx, out, *, coeff_ids=None, tally=None, agent=0, src_inp=None):
    """eng: the engine after the step of `inp` (agent `agent` of its last batch); res: that agent's result dict; fx: the loaded
    fixture `inp` was rebuilt from (collision=False); out: oracle.plan_step of the same inputs, read for margin / frag_sites /
    planes-as-conditioning only; src_inp: the oracle's inputs (its own hull builder) for admissible_outcomes.  Returns this
    call's tally (and adds it to `tally`)."""
    from oracle import oracle
    t = new_tally()
    t["calls"] = 1
    robust = out["margin"] >= FRAGILE
    n = len(robust)
    assert res["n_candidates"] == n == len(fx["valid"])
    n_frag = int((~robust).sum())
    cost, flags = eng.costs(agent)
    have_reasons = fx["hist"][0] >= 0
    t["checked"], t["nonrobust"] = n, n_frag

    # -- decisions --
    bit = lambda b: (flags & b) != 0
    valid_dev, feas_dev, ret_dev, costed_dev = (bit(_abi.FX_FLAG_VALID), bit(_abi.FX_FLAG_FEASIBLE), bit(_abi.FX_FLAG_RETURNED),
                                                bit(_abi.FX_FLAG_COSTED))
    reasons_dev = (flags >> _abi.FX_REASON_SHIFT) & 0x7FF
    assert np.array_equal(valid_dev[robust], fx["valid"][robust]), "valid"
    assert np.array_equal(ret_dev[robust], fx["returned"][robust]), "returned"
    assert np.array_equal(costed_dev[robust], fx["costed"][robust]), "costed"
    ret = fx["returned"] & robust
    assert np.array_equal(feas_dev[ret], fx["feasible"][ret]), "feasible"
    if have_reasons:
        bad = np.nonzero(robust & (reasons_dev != fx["reasons"]))[0]
        assert not len(bad), f"reason bits of candidate {bad[0]}: {int(reasons_dev[bad[0]]):#x}, the reference's {int(fx['reasons'][bad[0]]):#x}"
    # counters: within the number of candidates the reference decides by the last ulp
    assert abs(res["n_returned"] - int(fx["returned"].sum())) <= n_frag, "n_returned"
    assert abs(res["n_feasible"] - int((fx["valid"] & fx["feasible"] & fx["returned"]).sum())) <= n_frag, "n_feasible"
    if have_reasons:
        assert np.abs(np.array(res["reason_hist"])[:len(fx["hist"])] - fx["hist"]).max() <= n_frag, "reason_hist"

    # -- conditioning of the reference's own arithmetic (the oracle's planes of the same inputs) --
    cond = conditioning_many(out["planes"])
    cond_kin = kinematic_conditioning_many(out["planes"])
    ill = cond_kin > WELL_CONDITIONED
    scaled = np.zeros(n, bool)

    # -- costs --
    names = [str(x) for x in fx["cost_names"]]
    cols = [list(inp.cost_names).index(x) for x in names]
    assert len(cols) == len(inp.cost_names)
    cm = eng.costmap(agent)[:, cols] if inp.write_costmap and len(names) else None
    c = fx["costed"] & costed_dev & robust
    if c.any():
        ref = fx["cost"]
        rel = np.zeros(n)
        rel[c] = np.abs(cost[c] - ref[c]) / np.maximum(np.abs(ref[c]), 1e-12)
        miss = c & ~(rel < COST_RTOL)
        bad = miss & ~(ill & (rel < COST_RTOL + 4e-14 * cond_kin))
        assert not bad.any(), (f"cost of candidate {np.nonzero(bad)[0][0]} off the reference's by {rel[bad].max():.3e} relative "
                               f"(conditioning {cond_kin[np.nonzero(bad)[0][0]]:.1e})")
        scaled |= miss
        t["max_cost"] = float(rel[c].max())
        if cm is not None:
            refm = fx["costmap"]
            relm = np.zeros(refm.shape)
            relm[c] = np.abs(cm[c] - refm[c]) / np.maximum(np.abs(refm[c]), 1e-9)
            missm = c[:, None] & ~(relm < COSTMAP_RTOL)
            kin = np.array([x in KINEMATIC_COSTS for x in names])
            door = ill[:, None] & kin[None, :] & (relm < COSTMAP_RTOL + 4e-14 * cond_kin[:, None])
            badm = missm & ~door
            assert not badm.any(), (f"cost term {names[np.argwhere(badm)[0][1]]} of candidate {np.argwhere(badm)[0][0]} off the "
                                    f"reference's by {relm[badm].max():.3e} relative")
            scaled |= missm.any(axis=1)
            t["max_costmap"] = float(relm[c].max())

    # -- coefficient rows, delta_tau, traj_len: robust or not --
    if coeff_ids is None:
        coeff_ids = coeff_ids_for(fx, robust)
    for g in np.asarray(coeff_ids, dtype=np.int64):
        g = int(g)
        lon, lat, tl, tau = eng.coeffs(g, agent)
        e_lon = float((np.abs(lon - fx["coeff_lon"][g]) / np.maximum(np.abs(fx["coeff_lon"][g]), 1e-3)).max())
        e_lat = float((np.abs(lat - fx["coeff_lat"][g]) / np.maximum(np.abs(fx["coeff_lat"][g]), 1e-3)).max())
        e_tau = abs(tau - fx["tau_lat"][g]) / abs(fx["tau_lat"][g])
        assert e_lon < COEFF_RTOL, f"coeff_lon of candidate {g} off the reference's by {e_lon:.3e}"
        assert e_lat < COEFF_RTOL, f"coeff_lat of candidate {g} off the reference's by {e_lat:.3e}"
        assert e_tau < COEFF_RTOL, f"tau_lat of candidate {g}: {tau}, the reference's {fx['tau_lat'][g]}"
        if fx["has_cart"][g]:
            assert tl == int(fx["traj_len"][g]), f"traj_len of candidate {g}: {tl}, the reference's {int(fx['traj_len'][g])}"
        t["max_coeff_lon"], t["max_coeff_lat"] = max(t["max_coeff_lon"], e_lon), max(t["max_coeff_lat"], e_lat)
        t["max_tau_lat"] = max(t["max_tau_lat"], float(e_tau))
    t["coeff_rows"] = len(coeff_ids)

    # -- order of the costed candidates: the reference's stable sort --
    sel = costed_dev & robust
    ids = np.nonzero(sel)[0]
    dev_sorted = ids[np.lexsort((ids, cost[ids]))]
    ref_sorted = np.array([g for g in fx["sorted_ids"] if sel[g]], dtype=np.int64)
    t["near_tie_ranks"] += _near_tie_ranks(ref_sorted, dev_sorted, fx["cost"], "order of the costed candidates")

    # -- the K best: the device's own (cost, index) order bit for bit, and the head of the reference's walk list --
    tc, ti = eng.topk(TOPK)
    tc, ti = tc[agent], ti[agent]
    elig = bit(_abi.FX_FLAG_SELECTABLE) & ~bit(_abi.FX_FLAG_COLLISION) & ~bit(_abi.FX_FLAG_BOUNDARY)
    eids = np.nonzero(elig)[0]
    own = eids[np.lexsort((eids, cost[eids]))][:TOPK]
    assert np.array_equal(ti[:len(own)], own), f"top-{TOPK} ids are not the (cost, index) order of the engine's own costs"
    assert np.array_equal(tc[:len(own)], cost[own]), f"top-{TOPK} costs are not the costs of those candidates"
    assert np.all(ti[len(own):] == -1)
    walk = fx["walk_ids"].astype(np.int64)
    dev_walk = np.array([g for g in ti if g >= 0 and robust[g]], dtype=np.int64)
    ref_walk = np.array([g for g in walk if robust[g]], dtype=np.int64)
    assert len(ref_walk) >= len(dev_walk), f"top-{TOPK} holds {len(dev_walk)} robust candidates, the reference's walk list {len(ref_walk)}"
    if n_frag == 0:
        assert len(dev_walk) == min(TOPK, len(walk))
    t["near_tie_ranks"] += _near_tie_ranks(ref_walk[:len(dev_walk)], dev_walk, fx["cost"], f"top-{TOPK} against the walk list")

    # -- winner --
    want = int(walk[0]) if len(walk) else -1
    best = int(res["best_index"])
    if best != want:
        t["winner_differs"] = 1
        if want >= 0:
            assert not robust[want], f"winner {best}, the reference's {want} (robust)"
        else:
            assert best >= 0 and not robust[best], f"winner {best} where the reference's walk list is empty"

    # -- planes of the stored subset and of every non-robust candidate --
    pids = fx["plane_ids"].astype(np.int64)
    pos = {int(g): k for k, g in enumerate(pids)}
    frag_ids = np.nonzero(~robust)[0]
    gids = np.unique(np.concatenate([pids, frag_ids])) if inp.write_bundle else np.zeros(0, np.int64)
    gpos = {int(g): k for k, g in enumerate(gids)}
    got = gather_planes(eng, gids, agent) if len(gids) else None

    def plane_err(g):
        ref = fx["planes"][pos[g]]
        return float((np.abs(got[gpos[g]] - ref) / (1.0 + np.abs(ref).max(axis=1, keepdims=True))).max())

    if got is not None:
        for g in pids:
            g = int(g)
            if not (robust[g] and fx["has_cart"][g]):
                continue
            e = plane_err(g)
            if not e < STATE_TOL:
                assert ill[g] and e < STATE_TOL + 2e-14 * cond[g], \
                    f"planes of candidate {g} off the reference's by {e:.3e} (conditioning {cond_kin[g]:.1e})"
                scaled[g] = True
            t["max_plane"] = max(t["max_plane"], e)

    # -- non-robust candidates: the fixture's outcome under the rules above, or another admissible one; none skipped --
    w_pl, _ = path_length_weight(inp)
    src = src_inp if src_inp is not None else inp
    for g in frag_ids:
        g = int(g)
        same = (valid_dev[g] == fx["valid"][g] and ret_dev[g] == fx["returned"][g] and costed_dev[g] == fx["costed"][g]
                and (not fx["returned"][g] or feas_dev[g] == fx["feasible"][g])
                and (not have_reasons or reasons_dev[g] == fx["reasons"][g]))
        if same and fx["costed"][g]:
            same = abs(cost[g] - fx["cost"][g]) < COST_RTOL * max(abs(fx["cost"][g]), 1e-12)
            if same and cm is not None:
                same = bool((np.abs(cm[g] - fx["costmap"][g]) < COSTMAP_RTOL * np.maximum(np.abs(fx["costmap"][g]), 1e-9)).all())
        if same and got is not None and g in pos and fx["has_cart"][g]:
            same = plane_err(g) < STATE_TOL + 2e-14 * cond[g]
        if same:
            t["nonrobust_fixture"] += 1
            continue
        outs = oracle.admissible_outcomes(src, g, out["frag_sites"][g])
        stored = bool(ret_dev[g]) and (bool(costed_dev[g]) or inp.draw_traj_set)
        ok = matches_one_outcome(outs, flags[g], cost[g] if costed_dev[g] else None, got[gpos[g]] if got is not None else None,
                                 cost_rtol=COST_RTOL, state_tol=FRAGILE_STATE_TOL, planes_stored=stored, path_length=(abs(w_pl), inp.dt))
        assert ok, (f"non-robust candidate {g} (sites {[oracle.SITES[k] for k in range(len(oracle.SITES)) if (out['frag_sites'][g] >> k) & 1]}): "
                    f"flags {hex(int(flags[g]))} / cost {cost[g]} are neither the fixture's outcome nor one of {[hex(o['flags']) for o in outs]}")
        t["nonrobust_other"] += 1
    assert t["nonrobust_fixture"] + t["nonrobust_other"] == n_frag

    t["scaled"] = int(scaled.sum())
    t["scaled_ids"] = [int(g) for g in np.nonzero(scaled)[0]]
    if tally is not None:
        add_tally(tally, t)
    return t
