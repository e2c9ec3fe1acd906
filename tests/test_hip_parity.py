"""Parity of the HIP engine (through the C-ABI, libfxplan.so) against the CPU oracle on a real MI355X.

Bit-exact on every index / mask / counter, floating-point planes within 1e-9 (the north-star bound on Cartesian states is
1e-6), costs within 1e-9 relative -- for EVERY candidate.  Two refinements instead of exclusions (tests/admissible.py):
candidates whose decisions the reference takes by the last ulp (oracle margin < FRAGILE) must equal one of the outcomes those
decisions admit, and where the reference's own cos(arctan(d')) loses digits (theta_cl next to pi/2) the tolerances grow with
sec(theta_cl).
"""
import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, synthetic
from tests.fixtures import golden_names, inputs_from_fixture, load_golden

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-9
COST_RTOL = 1e-9
FRAGILE = 1e-9
# How the candidates of every compare() were checked (tests/admissible.py): the tolerances grow with the conditioning of the
# reference's own arithmetic, and a tolerance of 1 or more leaves only the order of magnitude to assert -- so the suite counts what went through
# each door and fails when more than a sliver did: a regression in the arithmetic cannot hide behind the scaling.
#   checked      candidates compared                      fixed    well-conditioned (cond <= 1e3): asserted at 1e-9 (+ 2 %)
#   scaled       cond > 1e3: conditioning-scaled tolerance  escaped  some plane's tolerance >= 1: that plane carries no digit in the
#   fragile      decided by the last ulp: compared with every     reference either (theta_cl = pi/2 to the last bit: v = x / cos with
#                admissible outcome                                cos = rounding noise) -- asserted to its ORDER OF MAGNITUDE only
PARITY_STATS = dict(checked=0, fixed=0, scaled=0, escaped=0, fragile=0, fragile_same=0)
WELL_CONDITIONED = 1e3
MAX_ESCAPED_FRACTION = 1e-2     # per compare(): at most this share of the stored candidates (or 2 of them) asserted to magnitude only
#                                 (a (t, v) pair that drives backwards from standstill in LOW_VEL_MODE takes its ~10 lateral siblings along:
#                                 tools/soak_case.py, round-3 soak case 920156: 9 of 1 260, d' = 1e16, v = 1e29): the bound is on such PAIRS per case; the soak bounds the
#                                 candidates of a whole run at 5e-4
# raw cost terms formed from the planes that divide by cos(theta_cl) (v, a): conditioning-scaled tolerance; all others fixed
KINEMATIC_COSTS = ("velocity_offset", "acceleration", "jerk", "path_length")
NO_LEADING_DIGIT = 1e15         # conditioning from which cos(theta_cl) has not even a leading digit (1 / eps = 4.5e15)
MAGNITUDE_DECADES = 4.0         # what "order of magnitude" means for those planes: peak |value| within 10^+-4 of the oracle's, finite alike


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=120_000, max_steps=60, max_ref_knots=1024, max_obstacles=32, max_pred_steps=64,
                     max_agents=8)
    yield e
    e.close()


def hip_hulls():
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return build_obstacle_hulls


def settle_differing(ora, differ, flags, cost, limit=2000):
    """The large-grid tests compare with oracle.plan_range, which returns no margins: every candidate whose flag word differs is
    re-evaluated on its own (oracle.eval_forced), must have a decision the reference takes by the last ulp (a fragile site), and the
    device's (flags, cost) must equal ONE of the outcomes those decisions admit -- no candidate is exempt without that match."""
    from oracle import oracle
    from tests.admissible import matches_one_outcome
    ids = np.nonzero(differ)[0]
    assert len(ids) <= limit, f"{len(ids)} candidates differ from the oracle"
    for g in ids:
        o = oracle.eval_forced(ora, int(g))
        assert o["frag_sites"] != 0, f"candidate {g}: flag words differ ({flags[g]:#x} vs {o['flags']:#x}) without a fragile decision"
        outs = oracle.admissible_outcomes(ora, int(g), o["frag_sites"])
        assert matches_one_outcome(outs, flags[g], cost[g] if flags[g] & _abi.FX_FLAG_COSTED else None, None), \
            f"candidate {g}: device outcome {flags[g]:#x} / {cost[g]} is none of the {len(outs)} admissible ones"
    PARITY_STATS["fragile"] += len(ids)
    return len(ids)


def compare(eng, inp, out, res, *, check_planes=True, agent=0, ref_inp=None, xy_tol=None):
    """out = oracle.plan_step(ref_inp or inp) ; res = engine result of the same inputs.  EVERY candidate is checked:
      * decisions (flag word: masks + reasons) exactly, planes to STATE_TOL, costs to COST_RTOL -- where the reference itself
        loses digits (cos(arctan(d')) next to pi/2) the two tolerances grow with sec(theta_cl), tests/admissible.py;
      * candidates whose decisions the reference takes by the last ulp (oracle margin < FRAGILE) against every outcome those
        decisions admit: the device result must equal ONE of them.
    xy_tol (scenes far from the world origin, tests/test_frame_invariance_gpu.py): the planes are compared relative to 1 + their
    peak, which at UTM coordinates (5e6 m) lets (x, y) move by 5 mm -- while no arithmetic meets an ABSOLUTE 1e-9 m where
    np.spacing is 9.3e-10.  Given, xy_tol is the absolute bound in metres on the x and y planes of every stored candidate whose
    conditioning is ordinary, on top of everything else; None (every other call): nothing changes."""
    from oracle import oracle
    from tests.admissible import (FRAGILE_STATE_TOL, KINEMATIC_PLANES, conditioning_many, kinematic_conditioning_many, matches_one_outcome,
                                  path_length_weight, signed_integral_slack)
    robust = out["margin"] >= FRAGILE
    n_frag = int((~robust).sum())
    cost, flags = eng.costs(agent)
    # masks / reasons, exact
    for name, bit in (("valid", _abi.FX_FLAG_VALID), ("feasible", _abi.FX_FLAG_FEASIBLE),
                      ("returned", _abi.FX_FLAG_RETURNED), ("costed", _abi.FX_FLAG_COSTED),
                      ("selectable", _abi.FX_FLAG_SELECTABLE), ("collision", _abi.FX_FLAG_COLLISION)):
        got = (flags & bit) != 0
        assert np.array_equal(got[robust], out[name][robust]), name
    got_reasons = (flags >> _abi.FX_REASON_SHIFT) & 0x7FF
    assert np.array_equal(got_reasons[robust], out["reasons"][robust])
    if n_frag == 0:
        assert np.array_equal(flags, out["flags"])
    # counters
    ref = out["result"]
    assert abs(res["n_returned"] - ref["n_returned"]) <= n_frag
    assert abs(res["n_feasible"] - ref["n_feasible"]) <= n_frag
    assert np.abs(np.array(res["reason_hist"]) - np.array(ref["reason_hist"])).max() <= n_frag
    assert res["n_candidates"] == ref["n_candidates"]
    # per-candidate conditioning of the reference's own arithmetic (1 for ordinary candidates)
    cond = conditioning_many(out["planes"]) if out.get("planes") is not None else np.ones(len(flags))
    # the same without the cap, for what divides by cos(theta_cl): v, a, kappa, kappa_dot and the costs built on them
    cond_kin = kinematic_conditioning_many(out["planes"]) if out.get("planes") is not None else np.ones(len(flags))
    # costs
    c = out["costed"] & robust & ((flags & _abi.FX_FLAG_COSTED) != 0)
    cm = eng.costmap(agent) if inp.write_costmap and len(inp.cost_names) else None
    # path_length is a signed sum of v: an absolute slack where it cancels (tests/admissible.py::signed_integral_slack)
    w_pl, j_pl = path_length_weight(inp)
    slack = signed_integral_slack(out["planes"], inp.dt, STATE_TOL) if w_pl and out.get("planes") is not None else np.zeros(len(flags))
    if c.any():
        err = np.abs(cost[c] - out["cost"][c])
        rtol_c = COST_RTOL + 4e-14 * cond_kin[c]
        lim = rtol_c * np.maximum(np.abs(out["cost"][c]), 1e-12) + abs(w_pl) * slack[c]
        # a total that contains a term built on v or a carries no digit where that term carries none (relative tolerance >= 1,
        # the rule of the raw terms below): finiteness is what is left to compare.  (Case 2070349 of the 144 000-scenario soak:
        # a standstill start in LOW_VEL_MODE, theta_cl = pi/2 to the last bit, jerk 3.6e80 against 2.0e68 at a conditioning of
        # 1.6e16 -- the raw terms were accepted by that rule, the total was still held to 653 times its own size.)
        no_digit_c = (rtol_c >= 1.0) & bool(set(inp.cost_names) & set(KINEMATIC_COSTS))
        assert np.array_equal(np.isfinite(cost[c][no_digit_c]), np.isfinite(out["cost"][c][no_digit_c])), \
            "a total cost without digits is finite on one side only"
        PARITY_STATS["escaped_costs"] = PARITY_STATS.get("escaped_costs", 0) + int(no_digit_c.sum())
        assert (err < lim)[~no_digit_c].all(), f"cost rel err {(err / np.maximum(np.abs(out['cost'][c]), 1e-12))[~no_digit_c].max()}"
        # well-conditioned candidates without a signed-integral term: the FIXED relative bound
        wellc = (cond_kin[c] <= WELL_CONDITIONED) & (abs(w_pl) * slack[c] == 0)
        assert (err[wellc] < 1.05 * COST_RTOL * np.maximum(np.abs(out["cost"][c][wellc]), 1e-12)).all(), \
            "cost of a well-conditioned candidate beyond 1e-9 relative"
        if cm is not None:
            # raw terms: only those built on the planes that divide by cos(theta_cl) -- v and a -- get the conditioning-scaled
            # tolerance; every other term (jerk integrals of the coefficients, |d|, the prediction term on (x, y), theta_cl
            # itself) is held to the fixed 1e-8 whatever the candidate's conditioning.  Where the scaled relative tolerance
            # reaches 1 the reference's own term carries no digit (theta_cl = pi/2 to the last bit: v = x / cos with cos =
            # rounding noise, 1e15 m/s) and only finiteness is compared, as for the planes of such a candidate (found by the
            # round-4 soak, case 801049: velocity_offset 1.2e20 against 8.4e15 at a conditioning of 1.6e16, every other term
            # of the same candidate equal to 3e-16)
            errm = np.abs(cm[c] - out["costmap"][c])
            kin_cols = np.array([n in KINEMATIC_COSTS for n in inp.cost_names])
            rtolm = np.full(errm.shape, 1e-8)
            rtolm[:, kin_cols] += 4e-14 * cond_kin[c][:, None]
            limm = rtolm * np.maximum(np.abs(out["costmap"][c]), 1e-9)
            if j_pl is not None:
                limm[:, j_pl] += slack[c]
            no_digit = rtolm >= 1.0
            assert np.array_equal(np.isfinite(cm[c][no_digit]), np.isfinite(out["costmap"][c][no_digit])), \
                "a cost term without digits is finite on one side only"
            bad_m = (errm >= limm) & ~no_digit
            assert not bad_m.any(), f"costmap rel err {(errm / np.maximum(np.abs(out['costmap'][c]), 1e-9))[bad_m].max()}"
    # winner: identical unless a fragile candidate or a sub-tolerance cost gap is involved
    if res["best_index"] != ref["best_index"]:
        a, b = res["best_index"], ref["best_index"]
        involved = [g for g in (a, b) if g >= 0]
        gap = abs(out["cost"][a] - out["cost"][b]) if a >= 0 and b >= 0 else np.inf
        assert (not all(robust[g] for g in involved)) or gap < 1e-9 * max(1.0, abs(out["cost"][b])), (a, b, gap)
    else:
        if ref["best_index"] >= 0:
            assert abs(res["best_cost"] - ref["best_cost"]) <= COST_RTOL * max(1.0, abs(ref["best_cost"]))
        assert res["n_collisions"] == ref["n_collisions"] or n_frag > 0
    # planes
    got = None
    if check_planes and inp.write_bundle:
        stored = out["returned"] & robust & (out["costed"] | (inp.draw_traj_set))
        got = eng.bundle(agent)
        refp = out["planes"]
        errs = np.abs(got - refp) / (1.0 + np.abs(refp).max(axis=2, keepdims=True))   # [C, 14, S]
        if xy_tol is not None:
            xy_err = np.abs(got[:, :2] - refp[:, :2]).max(axis=(1, 2))
            ordinary = stored & (cond <= WELL_CONDITIONED)
            print(f"(x, y) absolute error {xy_err[ordinary].max():.3e} m (bound {xy_tol:.3e}, {int(ordinary.sum())} candidates)")
            assert (xy_err[ordinary] < xy_tol).all(), f"(x, y) off by {xy_err[ordinary].max()} m (bound {xy_tol})"
        # Steps that CRAWL (high-speed mode, s_dot between the "moving" literal 1e-3 and 1e-2 m/s): d'' = (d_ddot - d' s_ddot) / s_dot^2
        # divides the evaluation noise of two second derivatives -- sums of terms of order 1 .. 100 that cancel to 1e-4 at the end
        # of a stopping trajectory, 1e-15 .. 1e-14 absolute whatever their value -- by 1e-6 .. 1e-4.  The slowest sampled end
        # velocity is max(0.001, ...) (planner.py:304), so a seventh of a planner's candidates ends on such a step; their a, kappa
        # and kappa_dot there agree to ~3e-10 typically and, once in the 6.4e7 candidates of the round-4 soak, to 2.0e-9 (case
        # 1012012: 3.2 mm/s, horizon 5 s).  Those steps of those three planes get (1 / s_dot)^2 ulps of 2e-14 on top of the
        # fixed bound (2e-10 at 1 cm/s ... 2e-8 at 1 mm/s); every other step and plane of the candidate stays where it was.
        if not inp.low_vel_mode:
            sd = refp[:, 10, :]
            crawl = (sd > 1e-3) & (sd < 1e-2)
            crawl_next = crawl.copy()
            crawl_next[:, 1:] |= crawl[:, :-1]          # kappa_dot[i] = kappa[i] - kappa[i-1]
            with np.errstate(divide="ignore"):
                amp = np.where(crawl, 1.0 / (sd * sd), 0.0)
            amp_next = amp.copy()
            amp_next[:, 1:] = np.maximum(amp[:, 1:], amp[:, :-1])
            for pl, msk, am in ((4, crawl, amp), (5, crawl, amp), (6, crawl_next, amp_next)):
                e = errs[:, pl, :]
                over = stored[:, None] & msk & (e >= STATE_TOL + 2e-14 * am)
                assert not over.any(), f"plane {pl} err {e[over].max()} at a crawling step beyond 1e-9 + 2e-14 / s_dot^2"
                PARITY_STATS["crawl_steps"] = PARITY_STATS.get("crawl_steps", 0) + int((stored[:, None] & msk).sum())
                e[msk] = 0.0
        err = errs.max(axis=2)   # [C, 14]
        err[~stored] = 0
        tol = np.repeat((STATE_TOL + 2e-14 * cond)[:, None], err.shape[1], axis=1)
        tol[:, KINEMATIC_PLANES] = (STATE_TOL + 2e-14 * cond_kin)[:, None]
        bad = (err >= tol) & (tol < 1.0)   # a relative tolerance of 1 or more: the reference's own value carries no digit
        assert not bad.any(), (f"plane err {err[bad].max()} at (candidate, plane) {np.argwhere(bad)[0]} "
                               f"(tolerance {tol[bad][0]})")
        # well-conditioned candidates: the FIXED bound, whatever the scaling machinery says
        well = stored & (cond_kin <= WELL_CONDITIONED)
        assert not (err[well] >= 1.02 * STATE_TOL).any(), f"plane err {err[well].max()} on a well-conditioned candidate"
        esc_planes = stored[:, None] & (tol >= 1.0)
        if esc_planes.any():   # no digit to compare: both sides at least agree on finiteness and on the order of magnitude
            pk_ref, pk_dev = np.abs(refp).max(axis=2)[esc_planes], np.abs(got).max(axis=2)[esc_planes]
            fin = np.isfinite(pk_ref)
            assert np.array_equal(np.isfinite(pk_dev), fin), "a plane without digits is finite on one side only"
            # the order of magnitude is compared while cos(theta_cl) still has a leading digit; at a conditioning of 1 / eps
            # (theta_cl = pi/2 to the LAST bit: the cosine is rounding noise of either libm, 6e-17 or 1e-16 or 0) the quotient's
            # magnitude is arbitrary too and only finiteness is left (round-4 soak, case 801049: conditioning 1.6e16, v = 7e15
            # against 3e9 m/s)
            lead = (np.repeat(cond_kin[:, None], esc_planes.shape[1], axis=1)[esc_planes] < NO_LEADING_DIGIT)[fin]
            dec = np.abs(np.log10(np.maximum(pk_dev[fin], 1e-300) / np.maximum(pk_ref[fin], 1e-300)))
            assert (dec[lead] < MAGNITUDE_DECADES).all(), f"a plane without digits differs by {dec[lead].max():.1f} decades"
        escaped = esc_planes.any(axis=1)
        PARITY_STATS["checked"] += int(stored.sum())
        PARITY_STATS["fixed"] += int(well.sum())
        PARITY_STATS["scaled"] += int((stored & ~well).sum())
        PARITY_STATS["escaped"] += int(escaped.sum())
        # per case: a degenerate (t, v) pair takes its lateral siblings along (the ego rolls backwards from standstill in
        # LOW_VEL_MODE: ds/dt = 0 to the last bit at some step, every d of the pair hits theta_cl = pi/2 there), so what is
        # bounded per case is the number of such PAIRS; the number of candidates stays bounded over a whole run
        # (tests/test_soak_parity.py, tools/soak_parity.py: <= 5e-4 of everything checked)
        if inp.sampling_matrix is None:
            n_groups = len(set((np.nonzero(escaped)[0] // len(inp.d_samp)).tolist()))
        else:   # rows of the C x 13 matrix: (t1, ss1) identify the longitudinal polynomial
            rows = inp.sampling_matrix[np.nonzero(escaped)[0]]
            n_groups = len(set(zip(rows[:, 1].tolist(), rows[:, 5].tolist())))
        assert n_groups <= max(2, MAX_ESCAPED_FRACTION * stored.sum()), \
            f"{int(escaped.sum())} of {int(stored.sum())} candidates in {n_groups} (t, v) pairs have a plane whose tolerance reached 1 (magnitude only)"
        # coefficients / traj_len of a few candidates
        for g in np.linspace(0, inp.n_candidates - 1, 5).astype(int):
            lon, lat, tl, tau = eng.coeffs(int(g), agent)
            assert np.allclose(lon, out["coeff_lon"][g], rtol=1e-13, atol=0)
            assert np.allclose(lat, out["coeff_lat"][g], rtol=1e-13, atol=0)
            assert tl == out["traj_len"][g]
            assert abs(tau - out["tau_lat"][g]) <= 1e-13 * abs(out["tau_lat"][g])   # delta_tau of the lateral polynomial
            assert np.array_equal(eng.sample(int(g), agent), got[g])
    # fragile candidates: one of the admissible outcomes, nothing skipped
    PARITY_STATS["fragile"] += n_frag
    src = ref_inp if ref_inp is not None else inp
    for g in np.nonzero(~robust)[0]:
        # (how often the device took the very branches the reference's arithmetic took: the whole flag word equal)
        PARITY_STATS["fragile_same"] += int(int(flags[g]) == int(out["flags"][g]))
        outs = oracle.admissible_outcomes(src, int(g), out["frag_sites"][g])
        stored = bool(flags[g] & _abi.FX_FLAG_RETURNED) and (bool(flags[g] & _abi.FX_FLAG_COSTED) or inp.draw_traj_set)
        ok = matches_one_outcome(outs, flags[g], cost[g] if flags[g] & _abi.FX_FLAG_COSTED else None,
                                 got[g] if got is not None else None, cost_rtol=COST_RTOL, state_tol=FRAGILE_STATE_TOL,
                                 planes_stored=stored, path_length=(abs(w_pl), inp.dt))
        assert ok, (f"fragile candidate {g} (sites {[oracle.SITES[k] for k in range(len(oracle.SITES)) if (out['frag_sites'][g] >> k) & 1]}): "
                    f"device flags {hex(int(flags[g]))} match none of {[hex(o['flags']) for o in outs]}")


@pytest.mark.parametrize("name", golden_names())
def test_golden_cases_vs_oracle(eng, name):
    from oracle import oracle
    fx = load_golden(name)
    inp = inputs_from_fixture(fx, hip_hulls())
    ref_inp = inputs_from_fixture(fx, oracle.build_obstacle_hulls)
    if inp.obstacles["K"]:
        assert np.allclose(inp.obstacles["hull"], ref_inp.obstacles["hull"], rtol=0, atol=1e-12)
    out = oracle.plan_step(ref_inp)
    res = eng.plan_step(inp)
    compare(eng, inp, out, res, ref_inp=ref_inp)


@pytest.mark.parametrize("name", golden_names())
def test_golden_cases_vs_reference_vectors(eng, name):
    """HIP output against the reference's own vectors directly (not via the oracle), every stored candidate: within 1e-6 of the
    reference's planes (the north-star bound; 1e-9 for all but a handful) -- or, where the reference took a decision by the
    last ulp, equal to the oracle's outcome with that decision taken the other way."""
    from oracle import oracle
    from tests.admissible import FRAGILE_STATE_TOL, matches_one_outcome
    fx = load_golden(name)
    inp = inputs_from_fixture(fx, hip_hulls(), collision=False)
    ref_inp = inputs_from_fixture(fx, oracle.build_obstacle_hulls, collision=False)
    res = eng.plan_step(inp)
    if name in ("arc_hv_l4_horizon5_prod_obs8", "config3_grid_prod_obs20"):   # 22 440 candidates / BASELINE config 3 itself: config 3's decomposition, against the reference itself
        info = eng.step_info()
        assert info["lanes_per_candidate"] == 2 and info["wave_split"] == 1 and info["obstacle_kernel"] == 1 and not info["fused_selection"]
    cost, flags = eng.costs()
    ids = fx["plane_ids"]
    bundle = eng.bundle()
    got = bundle[ids]
    stored = fx["has_cart"][ids]
    err = (np.abs(got - fx["planes"]) / (1.0 + np.abs(fx["planes"]).max(axis=2, keepdims=True))).max(axis=(1, 2))
    err[~stored] = 0
    feas_gpu = (flags & _abi.FX_FLAG_FEASIBLE) != 0
    ret = fx["returned"]
    out = oracle.plan_step(ref_inp)
    robust = out["margin"] >= FRAGILE
    from tests.admissible import conditioning_many
    cond = conditioning_many(fx["planes"])
    # candidates without a fragile decision: the reference's own vectors to 1e-9 (scaled where the reference loses digits)
    rb = robust[ids]
    assert (err[rb] < STATE_TOL + 2e-14 * cond[rb]).all(), f"robust candidate off the reference's vectors by {err[rb].max()}"
    assert np.array_equal(feas_gpu[ret & robust], fx["feasible"][ret & robust])
    # fragile ones: same branch as the reference took (1e-6: the step on the threshold is ill-conditioned) or the other one
    suspects = set(int(g) for g in ids[(err > 1e-6) & ~rb]) | set(int(g) for g in np.nonzero(ret & ~robust & (feas_gpu != fx["feasible"]))[0])
    for g in sorted(suspects):
        outs = oracle.admissible_outcomes(ref_inp, g, out["frag_sites"][g])
        st = bool(flags[g] & _abi.FX_FLAG_RETURNED) and (bool(flags[g] & _abi.FX_FLAG_COSTED) or inp.draw_traj_set)
        assert matches_one_outcome(outs, flags[g], cost[g] if flags[g] & _abi.FX_FLAG_COSTED else None, bundle[g],
                                   state_tol=FRAGILE_STATE_TOL, planes_stored=st), g
    if len(fx["walk_ids"]):
        assert res["best_index"] == int(fx["walk_ids"][0])
    # the boundary attributes of the sample views (polynomial_trajectory.py:17-60): delta_tau of the lateral polynomial is the
    # reference's own (t at speed, s_lon_goal in LOW_VEL_MODE -- reactive_planner.py:161-171, :650-659), the longitudinal one's t
    from frenetix_motion_planner_amd.trajectories import PlanStepResult
    step = PlanStepResult(eng, inp, res)
    nVD = len(inp.v_samp) * len(inp.d_samp)
    for g in np.unique(np.concatenate([np.linspace(0, inp.n_candidates - 1, 24).astype(int), fx["walk_ids"][:1].astype(int)])):
        tr = step.sample(int(g))
        assert abs(tr.trajectory_lat.delta_tau - fx["tau_lat"][g]) <= 1e-10 * abs(fx["tau_lat"][g]), (name, g)
        assert tr.trajectory_long.delta_tau == inp.t_samp[int(g) // nVD]
        assert np.allclose(tr.trajectory_lat.coeffs, fx["coeff_lat"][g], rtol=1e-9, atol=1e-12)
    # ... and the packaged winner carries it too (fx_read_package)
    if len(fx["walk_ids"]):
        res2, pkg = eng.plan_step_packaged(inp)
        assert pkg is not None and pkg.index == int(fx["walk_ids"][0])
        assert abs(pkg.tau_lat - fx["tau_lat"][pkg.index]) <= 1e-10 * abs(fx["tau_lat"][pkg.index])


CASES = {
    "dense_debug_obs": dict(ref_kind="arc", v0=10.0, grid=(9, 21, 21), n_obstacles=8, draw_traj_set=True, kinematic_debug=True),
    "dense_prod_obs": dict(ref_kind="arc", v0=10.0, grid=(9, 21, 21), n_obstacles=20),
    "dense_prod_scurve": dict(ref_kind="scurve", kappa=0.03, v0=13.0, grid=(7, 15, 17), n_obstacles=6, seed=7),
    "dense_lowvel": dict(ref_kind="arc", v0=1.2, v_des=3.0, grid=(6, 11, 13), n_obstacles=3, seed=3),
    "dense_horizon5": dict(ref_kind="arc", n_knots=700, v0=11.0, grid=(12, 9, 11), horizon=5.0, n_pred=50, n_obstacles=5,
                           draw_traj_set=True, kinematic_debug=True),
    "allcosts": dict(ref_kind="scurve", v0=9.0, grid=(5, 9, 9), n_obstacles=4, draw_traj_set=True, kinematic_debug=True,
                     cost_weights=dict(acceleration=0.3, jerk=0.15, orientation_offset=0.4, path_length=0.05,
                                       lateral_jerk=0.2, longitudinal_jerk=0.2, velocity_offset=1.0,
                                       distance_to_reference_path=5.0, prediction=0.2)),
    # lane_center_offset (partial_cost_functions.py:91-117): own lane and left neighbour along the reference, nothing to the right
    "lane_center": dict(ref_kind="scurve", v0=9.0, grid=(5, 9, 9), n_obstacles=3, draw_traj_set=True, kinematic_debug=True,
                        lanelets=(3.5, 60), cost_weights=dict(lane_center_offset=2.0, lateral_jerk=0.2, velocity_offset=1.0,
                                                              prediction=0.2, distance_to_reference_path=1.0)),
    "lane_center_nolanes": dict(ref_kind="arc", v0=10.0, grid=(3, 5, 7), cost_weights=dict(lane_center_offset=1.0, jerk=0.1)),
    "ragged_tail": dict(ref_kind="arc", v0=10.0, grid=(3, 7, 13), n_obstacles=2),  # C not a multiple of 64
    "single_candidate": dict(ref_kind="arc", v0=10.0, grid=(1, 1, 1), d0=0.0),
    "no_costs": dict(ref_kind="arc", v0=10.0, grid=(3, 5, 5), cost_weights={}),
    # stop-point sampling: end positions instead of end velocities, longitudinal quintic (reactive_planner.py:628-671)
    "stop_dense_obs": dict(ref_kind="arc", v0=7.0, grid=(9, 21, 21), stop_point_s=30.0, v_des=0.0, n_obstacles=4),
    "stop_lowvel_debug": dict(ref_kind="arc", v0=1.5, grid=(6, 11, 13), stop_point_s=6.0, v_des=0.0, draw_traj_set=True,
                              kinematic_debug=True),
    "stop_scurve_kd": dict(ref_kind="scurve", kappa=0.02, v0=9.0, grid=(7, 15, 17), stop_point_s=35.0, v_des=0.0,
                           kinematic_debug=True, seed=5),
    # the other readings of CCosy's projection: d along the un-normalised interpolated normal
    # (FX_MODE_PROJ_PSEUDO_NORMAL), vertex tangents from the bisector of the adjacent segments -- tight curve, jittered knots
    "proj_pseudo_normal": dict(ref_kind="arc", kappa=0.05, knot_jitter=0.3, v0=8.0, grid=(7, 11, 13), n_obstacles=4,
                               draw_traj_set=True, kinematic_debug=True, pseudo_normal=True),
    "proj_pseudo_bisector_prod": dict(ref_kind="arc", kappa=0.05, knot_jitter=0.3, v0=8.0, grid=(7, 11, 13), n_obstacles=4,
                                      pseudo_normal=True, vertex_tangent="bisector"),
    "proj_bisector": dict(ref_kind="arc", kappa=0.05, knot_jitter=0.3, v0=8.0, grid=(7, 11, 13), n_obstacles=4,
                          draw_traj_set=True, kinematic_debug=True, vertex_tangent="bisector"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_synthetic_cases_vs_oracle(eng, name):
    from oracle import oracle
    kw = CASES[name]
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    ref_inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
    out = oracle.plan_step(ref_inp)
    res = eng.plan_step(inp)
    compare(eng, inp, out, res, ref_inp=ref_inp)
    if name == "dense_prod_obs":
        # a meaningful share of otherwise-best candidates must collide
        assert out["collision"].sum() > 0
    if name == "proj_pseudo_normal":
        # the variant is not a no-op: against the default projection the (x, y) planes move by more than the north star's 1e-6 m
        base = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **dict(kw, pseudo_normal=False)))
        m = out["returned"] & out["costed"] & base["returned"] & base["costed"]
        assert np.abs(out["planes"][m][:, :2] - base["planes"][m][:, :2]).max() > 1e-5


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("wpe", [2, 3, 4])
@pytest.mark.parametrize("name", ["dense_debug_obs", "dense_prod_obs", "dense_lowvel", "dense_horizon5", "ragged_tail",
                                  "single_candidate", "stop_dense_obs", "stop_lowvel_debug"])
def test_work_decomposition_does_not_change_results(eng, name, lanes, wpe, variant):
    """Every (kernel variant, lanes per candidate, occupancy target) specialisation against the oracle."""
    from oracle import oracle
    kw = CASES[name]
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    eng.set_tuning(lanes, wpe, variant)
    try:
        try:
            res = eng.plan_step(inp)
        except ValueError as e:
            if "not applicable" in str(e):
                pytest.skip("grid kernel not applicable to this case (LDS budget)")
            raise
        compare(eng, inp, out, res)
    finally:
        eng.set_tuning(0, 0, 0)


@pytest.mark.parametrize("matrix", [False, True])
@pytest.mark.parametrize("lanes", [16, 32])
@pytest.mark.parametrize("name", sorted(CASES))
def test_one_or_two_steps_per_lane(eng, name, lanes, matrix):
    """16 / 32 lanes per candidate (planner-sized grids: every lane walks one or two steps plus its carry-in step; horizons
    shorter than the lane count leave parts without a step) against the oracle, on every synthetic case: sampling ranges (grid
    kernel where it applies) and the same candidates as a C x 13 sampling matrix (generic kernel)."""
    from oracle import oracle
    kw = dict(CASES[name])
    if matrix:
        if "stop_point_s" in kw or kw.get("as_matrix"):
            pytest.skip("stop-point sampling has no matrix form / the case is a matrix already")
        kw["as_matrix"] = True
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    eng.set_tuning(lanes, 2, 0)
    try:
        res = eng.plan_step(inp)
        info = eng.step_info()
        windowed = set(inp.cost_names) & {"acceleration", "jerk", "orientation_offset", "path_length", "distance_to_obstacles",
                                               "lane_center_offset"}
        assert info["lanes_per_candidate"] == (1 if windowed else lanes)   # windowed costs keep the horizon in one lane
        compare(eng, inp, out, res)
    finally:
        eng.set_tuning(0, 0, 0)


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("wpe", [2, 4])
@pytest.mark.parametrize("name", ["dense_debug_obs", "dense_prod_obs", "dense_lowvel", "dense_horizon5", "ragged_tail",
                                  "single_candidate", "dense_prod_scurve"])
def test_wave_split_mapping(eng, name, lanes, wpe):
    """Parts of a candidate on different lane-groups of the workgroup (LDS combine) against the oracle."""
    from oracle import oracle
    kw = CASES[name]
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    eng.set_tuning(lanes, wpe, 2, 256, 2)
    try:
        try:
            res = eng.plan_step(inp)
        except ValueError as e:
            if "not applicable" in str(e):
                pytest.skip("grid kernel / wave split not applicable to this case")
            raise
        compare(eng, inp, out, res)
    finally:
        eng.set_tuning(0, 0, 0, 0, 0)


@pytest.mark.parametrize("lanes", [2, 4])
@pytest.mark.parametrize("name", ["short_ref_hv_l1_debug", "arc_standstill_l1_debug", "arc_slow_brake_l1_kd", "scurve_hv_l2_kd"])
def test_wave_split_on_golden_cases(eng, name, lanes):
    from oracle import oracle
    fx = load_golden(name)
    inp = inputs_from_fixture(fx, hip_hulls())
    out = oracle.plan_step(inputs_from_fixture(fx, oracle.build_obstacle_hulls))
    eng.set_tuning(lanes, 0, 2, 256, 2)
    try:
        try:
            res = eng.plan_step(inp)
        except ValueError as e:
            if "not applicable" in str(e):
                pytest.skip("grid kernel / wave split not applicable to this case")
            raise
        compare(eng, inp, out, res)
    finally:
        eng.set_tuning(0, 0, 0, 0, 0)


@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["short_ref_hv_l1_debug", "arc_standstill_l1_debug", "arc_slow_brake_l1_kd",
                                  "arc_hv_l2_debug_obs5", "scurve_hv_l2_kd", "arc_lv_l1_debug"])
def test_split_horizon_on_golden_cases(eng, name, lanes, variant):
    """Projection-domain exits, standstill heading carry and first-violation semantics across chunk borders."""
    from oracle import oracle
    fx = load_golden(name)
    inp = inputs_from_fixture(fx, hip_hulls())
    out = oracle.plan_step(inputs_from_fixture(fx, oracle.build_obstacle_hulls))
    eng.set_tuning(lanes, 0, variant)
    try:
        try:
            res = eng.plan_step(inp)
        except ValueError as e:
            if "not applicable" in str(e):
                pytest.skip("grid kernel not applicable to this case (LDS budget)")
            raise
        compare(eng, inp, out, res)
    finally:
        eng.set_tuning(0, 0, 0)


@pytest.mark.parametrize("stop", [None, 28.0])
def test_generic_and_grid_kernels_agree_bitwise(eng, stop):
    """Same walk, two kernels: every flag, plane, counter and cost term is bit-identical -- except the prediction cost, which
    the grid kernel evaluates through the Cholesky factor of the inverse covariance from its staged obstacle table
    (fx_walk.h, ObsHot) and the generic kernel in the reference's r0 e0 + r1 e1 form: equal to rounding."""
    kw = dict(ref_kind="scurve", kappa=0.02, v0=9.0, grid=(7, 9, 33), n_obstacles=6, draw_traj_set=True, kinematic_debug=True,
              stop_point_s=stop)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    outs = []
    try:
        for variant in (1, 2):
            eng.set_tuning(1, 0, variant)
            res = eng.plan_step(inp)
            outs.append((res, *eng.costs(), eng.bundle(), eng.costmap()))
    finally:
        eng.set_tuning(0, 0, 0)
    a, b = outs
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    ip = inp.cost_names.index("prediction")
    others = [n for n in range(len(inp.cost_names)) if n != ip]
    assert np.array_equal(a[4][:, others], b[4][:, others])
    assert np.allclose(a[4][:, ip], b[4][:, ip], rtol=1e-12, atol=0)
    assert np.allclose(a[1], b[1], rtol=1e-12, atol=0)
    assert a[0]["best_index"] == b[0]["best_index"] and a[0]["reason_hist"] == b[0]["reason_hist"]


def test_sampling_matrix_mode_matches_ranges(eng):
    kw = dict(ref_kind="arc", v0=10.0, grid=(5, 9, 11), n_obstacles=4)
    a = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    b = synthetic.make_inputs(hull_builder=hip_hulls(), as_matrix=True, **kw)
    eng.set_tuning(8, 0, 0)   # the same horizon split on both kernels: the cost sums associate identically -> bitwise
    try:
        ra = eng.plan_step(a)
        ca, fa = eng.costs()
        pa = eng.bundle()
        rb = eng.plan_step(b)
        cb, fb = eng.costs()
        pb = eng.bundle()
    finally:
        eng.set_tuning(0, 0, 0)
    assert np.array_equal(fa, fb) and np.array_equal(ca, cb) and np.array_equal(pa, pb)
    for k in ("best_index", "best_cost", "n_returned", "n_feasible", "n_collisions", "reason_hist"):
        assert ra[k] == rb[k]


def test_select_only_mode_equals_bundle_mode(eng):
    kw = dict(ref_kind="arc", v0=10.0, grid=(5, 9, 11), n_obstacles=4)
    a = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    b = synthetic.make_inputs(hull_builder=hip_hulls(), write_bundle=False, write_costmap=False, **kw)
    ra = eng.plan_step(a)
    ca, fa = eng.costs()
    rb = eng.plan_step(b)
    cb, fb = eng.costs()
    assert np.array_equal(fa, fb) and np.array_equal(ca, cb)
    assert ra["best_index"] == rb["best_index"] and ra["best_cost"] == rb["best_cost"]
    with pytest.raises(Exception):
        eng.sample(0)


RESULT_KEYS = ("best_index", "best_cost", "n_returned", "n_feasible", "n_infeasible", "n_collisions", "reason_hist",
               "n_candidates", "feasible_percentage")


@pytest.mark.parametrize("lanes", [0, 1, 4])
@pytest.mark.parametrize("name", ["dense_debug_obs", "dense_lowvel", "ragged_tail", "single_candidate", "no_costs",
                                  "dense_prod_obs"])
def test_fused_selection_equals_selection_kernel(eng, name, lanes):
    """The last-workgroup reduction inside the evaluation kernel and the separate selection kernel publish the
    same result block; repeated steps start from clean counters (ticket and histogram reset)."""
    kw = dict(CASES[name], collision=False)  # the collision-ordered count keeps the selection kernel
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    eng.set_tuning(lanes, 0, 0)
    try:
        eng.set_fused_selection(False)
        ref = eng.plan_step(inp)
        eng.set_fused_selection(True)
        for _ in range(3):
            got = eng.plan_step(inp)
            for k in RESULT_KEYS:
                assert got[k] == ref[k], k
        # evaluate() re-enqueued on resident inputs, several in a row before one finish
        eng.upload(inp)
        for _ in range(4):
            eng.evaluate()
        got = eng.finish()[0]
        for k in RESULT_KEYS:
            assert got[k] == ref[k], k
    finally:
        eng.set_fused_selection(True)
        eng.set_tuning(0, 0, 0)


@pytest.mark.parametrize("lanes", [0, 1, 4, 32])
@pytest.mark.parametrize("name", ["dense_debug_obs", "dense_prod_obs", "dense_prod_scurve", "dense_lowvel", "dense_horizon5", "allcosts"])
def test_fused_tail_counts_collisions_and_gathers_the_package(eng, name, lanes):
    """One launch per step WITH the collision stage and the winner package (fx_tail.h): the agent's last workgroup counts the
    colliding candidates in front of the winner (planner.py:336-357) and gathers the chosen trajectory itself.  Result block,
    package block, coefficients and raw costs equal what the selection kernel (+ its gather) publishes, and the oracle's
    collision count; repeated steps start from clean counters."""
    from oracle import oracle
    kw = dict(CASES[name])
    kw.setdefault("n_obstacles", 6)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    assert inp.collision and inp.obstacles["K"] > 0
    want = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw), want_planes=False)["result"]
    extra = any(n in inp.cost_names for n in ("acceleration", "jerk", "orientation_offset", "path_length", "distance_to_obstacles"))
    eng.set_tuning(0 if extra else lanes, 0, 0)
    eng.set_obstacle_stage(1)   # (the obstacle stage inside the evaluation kernel: what planner-sized steps run)
    try:
        eng.set_fused_selection(False)
        ref, ref_pkg = eng.plan_step_packaged(inp, yaw_rate0=0.25)
        info = eng.step_info()
        assert not info["fused_selection"] and info["tail"] == 0
        assert ref["n_collisions"] == want["n_collisions"] and ref["best_index"] == want["best_index"]
        eng.set_fused_selection(2)
        eng.upload(inp)   # (the choice is taken at upload time)
        eng._resident_key = None
        for rep in range(3):
            got, pkg = eng.plan_step_packaged(inp, yaw_rate0=0.25)
            info = eng.step_info()
            # the tail lives in the planner-sized decompositions (>= 4 lanes per candidate) and in the windowed-cost kernel; a
            # forced one-lane decomposition keeps the selection kernel
            in_kernel = info["lanes_per_candidate"] >= 4 or extra
            assert (info["fused_selection"], info["tail"]) == ((1, 3) if in_kernel else (0, 0)), info
            for k in RESULT_KEYS:
                assert got[k] == ref[k], (k, rep)
            assert (pkg is None) == (ref_pkg is None)
            if pkg is not None:
                assert pkg.index == ref_pkg.index and pkg.cost == ref_pkg.cost and pkg.flags == ref_pkg.flags
                assert pkg.traj_len == ref_pkg.traj_len and pkg.tau_lat == ref_pkg.tau_lat
                assert np.array_equal(pkg.block, ref_pkg.block)
                assert np.array_equal(pkg.lon, ref_pkg.lon) and np.array_equal(pkg.lat, ref_pkg.lat)
                assert np.array_equal(pkg.raw_costs, ref_pkg.raw_costs)
        # without the package: the count alone (tail = 1), several evaluations in a row before one finish
        eng.upload(inp)
        for _ in range(3):
            eng.evaluate()
        got = eng.finish()[0]
        assert eng.step_info()["tail"] == (1 if in_kernel else 0)
        for k in RESULT_KEYS:
            assert got[k] == ref[k], k
    finally:
        eng.set_fused_selection(True)
        eng.set_obstacle_stage(0)
        eng.set_tuning(0, 0, 0)
        eng._resident_key = None


def _walled_in(hull_builder, **kw):
    """inputs whose every candidate runs into a wall of five wide obstacles standing 7 m ahead across the whole road"""
    from frenetix_motion_planner_amd import pack_predictions
    inp = synthetic.make_inputs(hull_builder=hull_builder, n_obstacles=1, **kw)
    cs, s0 = inp.coordinate_system, float(inp.x0_lon[0])
    preds = {}
    for j, dd in enumerate(np.linspace(-5.0, 5.0, 5)):
        xy = np.array([cs.convert_to_cartesian_coords(s0 + 7.0, float(dd))] * 31, dtype=float)
        preds[j] = dict(pos_list=xy, cov_list=np.tile(np.eye(2) * 0.1, (31, 1, 1)), orientation_list=np.full(31, float(cs.ref_theta[cs.segment_of(s0 + 7.0)])),
                        shape=dict(length=4.0, width=3.5))
    inp.obstacles = pack_predictions(preds, inp.n_samples, hull_builder)
    inp.predictions = preds
    inp._skey = None
    return inp


def test_fused_tail_everything_collides_and_nothing_selectable(eng):
    """No collision-free candidate: every selectable candidate is counted, no winner, no package (`found` = 0); and a step in
    which nothing is selectable at all (an ego far above every velocity the constraints allow)."""
    from oracle import oracle
    cases = [("wall", dict(ref_kind="straight", v0=8.0, grid=(3, 5, 7))), ("infeasible", dict(ref_kind="arc", kappa=0.05, v0=40.0, v_des=40.0, grid=(3, 5, 5), n_obstacles=2))]
    for tag, kw in cases:
        if tag == "wall":
            inp, ref_inp = _walled_in(hip_hulls(), **kw), _walled_in(oracle.build_obstacle_hulls, **kw)
        else:
            inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
            ref_inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
        want = oracle.plan_step(ref_inp, want_planes=False)
        assert want["result"]["best_index"] == -1, tag
        if tag == "wall":
            assert want["result"]["n_collisions"] == int(want["selectable"].sum()) > 0
        else:
            assert int(want["selectable"].sum()) == 0
        eng.set_obstacle_stage(1)
        try:
            eng.set_fused_selection(2)
            eng._resident_key = None
            for _ in range(2):
                got, pkg = eng.plan_step_packaged(inp)
                assert eng.step_info()["tail"] == 3
                for k in ("best_index", "n_collisions", "n_feasible", "n_returned"):
                    assert got[k] == want["result"][k], (tag, k)
                assert pkg is None
        finally:
            eng.set_fused_selection(True)
            eng.set_obstacle_stage(0)
            eng._resident_key = None


def test_fused_selection_batch(eng):
    kws = [dict(ref_kind="arc", v0=10.0, grid=(5, 9, 11), seed=1),
           dict(ref_kind="scurve", kappa=0.02, v0=6.0, grid=(4, 7, 9), seed=2, draw_traj_set=True, kinematic_debug=True),
           dict(ref_kind="straight", v0=1.0, v_des=2.0, d0=0.0, grid=(1, 1, 1), seed=3),
           dict(ref_kind="arc", n_knots=300, v0=15.0, grid=(6, 11, 9), seed=4, write_bundle=False)]
    inps = [synthetic.make_inputs(**kw) for kw in kws]
    eng.set_fused_selection(False)
    try:
        ref = eng.plan_batch(inps)
    finally:
        eng.set_fused_selection(True)
    for _ in range(2):
        got = eng.plan_batch(inps)
        for a in range(len(inps)):
            for k in RESULT_KEYS:
                assert got[a][k] == ref[a][k], (a, k)


def test_stop_point_sampling_rejects_a_matrix(eng):
    inp = synthetic.make_inputs(ref_kind="arc", v0=7.0, grid=(3, 5, 5), as_matrix=True)
    with pytest.raises(ValueError):
        inp.stop_point = True
        inp.__post_init__()
    st = inp.as_struct()
    st.lon_mode = _abi.FX_LON_STOP_POINT
    arr = (_abi.FxProblem * 1)(st)
    from frenetix_motion_planner_amd._lib import lib
    assert lib().fx_upload_batch(eng._ctx, 1, arr) < 0  # FX_ERR_INVALID_ARGUMENT
    st.lon_mode = 7
    arr = (_abi.FxProblem * 1)(st)
    assert lib().fx_upload_batch(eng._ctx, 1, arr) < 0


def test_topk_is_sorted_prefix(eng):
    from oracle import oracle
    kw = dict(ref_kind="arc", v0=10.0, grid=(7, 13, 13), n_obstacles=10)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    res = eng.plan_step(inp)
    cost, flags = eng.costs()
    k = 32
    tc, ti = eng.topk(k)
    ok = ((flags & _abi.FX_FLAG_SELECTABLE) != 0) & ((flags & _abi.FX_FLAG_COLLISION) == 0)
    ids = np.nonzero(ok)[0]
    order = ids[np.lexsort((ids, cost[ids]))][:k]
    assert np.array_equal(ti[0][:len(order)], order)
    assert np.array_equal(tc[0][:len(order)], cost[order])
    assert ti[0][0] == res["best_index"]
    assert np.all(ti[0][len(order):] == -1)


def test_batch_of_agents_equals_individual_steps(eng):
    kws = [dict(ref_kind="arc", v0=10.0, grid=(5, 9, 11), n_obstacles=4, seed=1),
           dict(ref_kind="scurve", kappa=0.02, v0=6.0, grid=(4, 7, 9), n_obstacles=2, seed=2, draw_traj_set=True,
                kinematic_debug=True),
           dict(ref_kind="straight", v0=1.0, v_des=2.0, d0=0.0, grid=(3, 5, 5), seed=3),
           dict(ref_kind="arc", n_knots=300, v0=15.0, grid=(6, 11, 9), n_obstacles=7, seed=4, write_bundle=False)]
    inps = [synthetic.make_inputs(hull_builder=hip_hulls(), **kw) for kw in kws]
    singles = []
    for inp in inps:
        r = eng.plan_step(inp)
        singles.append((r, *eng.costs()))
    batch = eng.plan_batch(inps)
    for a, (r, c, f) in enumerate(singles):
        cb, fb = eng.costs(a)
        assert np.array_equal(c, cb) and np.array_equal(f, fb)
        for k in ("best_index", "best_cost", "n_returned", "n_feasible", "n_collisions", "reason_hist", "n_candidates"):
            assert batch[a][k] == r[k], (a, k)
    assert np.array_equal(eng.sample(3, 1).shape, (14, 31))


def test_error_conventions(eng):
    inp = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(2, 3, 3))
    st = inp.as_struct()
    st.N = 0
    from frenetix_motion_planner_amd._lib import lib, check
    import ctypes as C
    res = _abi.FxResult()
    with pytest.raises(ValueError):
        check(lib().fx_plan_step(eng._ctx, C.byref(st), C.byref(res)))
    big = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(19, 120, 120))
    with pytest.raises(ValueError):  # capacity exceeded -> negative status -> ValueError
        eng.plan_step(big)
    # the context stays usable
    assert eng.plan_step(inp)["n_candidates"] == inp.n_candidates


def test_config2_full_size_properties():
    """BASELINE config 2 at full size (50 388 x 31, no obstacles): size-independent properties."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    inp = synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(19, 51, 51), hull_builder=hip_hulls())
    assert inp.n_candidates == 50388
    with FrenetEngine(max_candidates=inp.n_candidates) as e:
        res = e.plan_step(inp)
        cost, flags = e.costs()
        sel = ((flags & _abi.FX_FLAG_SELECTABLE) != 0)
        # winner is the lexicographic (cost, index) minimum of the selectable set
        ids = np.nonzero(sel)[0]
        best = ids[np.lexsort((ids, cost[ids]))][0]
        assert res["best_index"] == best and res["best_cost"] == cost[best]
        # counters are consistent with the flag words
        assert res["n_returned"] == int(((flags & _abi.FX_FLAG_RETURNED) != 0).sum())
        assert res["n_feasible"] == int((((flags & 3) == 3) & ((flags & _abi.FX_FLAG_RETURNED) != 0)).sum())
        # idempotence
        res2 = e.plan_step(inp)
        c2, f2 = e.costs()
        assert np.array_equal(c2, cost) and np.array_equal(f2, flags) and res2["best_index"] == res["best_index"]
        # s is non-decreasing for valid candidates; kappa_dot is the first difference of kappa
        s_pl, k_pl, kd_pl = e.plane("s"), e.plane("kappa"), e.plane("kappa_dot")
        valid = (flags & _abi.FX_FLAG_VALID) != 0
        assert np.all(np.diff(s_pl[:, valid], axis=0) >= -1e-4)
        assert np.array_equal(kd_pl[1:], k_pl[1:] - k_pl[:-1])
        # spot-check 600 candidates against the oracle
        out = oracle.plan_step(synthetic.make_inputs(ref_kind="arc", v0=10.0, grid=(19, 51, 51)), want_planes=False)
        robust = out["margin"] >= FRAGILE
        assert np.array_equal(flags[robust], out["flags"][robust])
        c = out["costed"] & robust
        assert (np.abs(cost[c] - out["cost"][c]) / np.maximum(np.abs(out["cost"][c]), 1e-12)).max() < COST_RTOL
        assert res["best_index"] == out["result"]["best_index"]


def test_config3_full_size_vs_oracle():
    """BASELINE config 3 at full size (50 388 x 31, 20 predicted obstacles, collision stage): every candidate against
    the oracle; the generator's promise that a good share of the otherwise-best candidates collide."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    kw = dict(ref_kind="arc", v0=10.0, grid=(19, 51, 51), n_obstacles=20, n_pred=30, lead_gap=25.0)  # = bench.py config3
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw), want_planes=False)
    with FrenetEngine(max_candidates=inp.n_candidates) as e:
        for select_only in (False, True):
            inp.write_bundle = inp.write_costmap = not select_only
            res = e.plan_step(inp)
            cost, flags = e.costs()
            robust = out["margin"] >= FRAGILE
            assert np.array_equal(flags[robust], out["flags"][robust])
            c = out["costed"] & robust
            assert (np.abs(cost[c] - out["cost"][c]) / np.maximum(np.abs(out["cost"][c]), 1e-12)).max() < COST_RTOL
            assert res["best_index"] == out["result"]["best_index"] and res["n_collisions"] == out["result"]["n_collisions"]
            if not select_only:
                # the planes of the bench-sized bundle: every 64th candidate (and the winner) against the oracle's forced-decision
                # evaluation of that one candidate, at the fixed tolerance where the reference's own values carry digits
                from tests.admissible import conditioning_many
                ref_inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
                ids = np.unique(np.concatenate([np.arange(0, inp.n_candidates, 64), [res["best_index"]]]))
                ids = ids[robust[ids] & out["returned"][ids] & out["costed"][ids]]
                assert len(ids) > 300
                want = np.stack([oracle.eval_forced(ref_inp, int(g))["planes"] for g in ids])
                got = np.stack([e.sample(int(g)) for g in ids[:8]])
                bundle_rows = np.stack([e.plane(p)[:, ids].T for p in range(_abi.FX_NUM_PLANES)], axis=1)   # [len(ids), 14, S]
                assert np.array_equal(bundle_rows[:8], got)
                err = np.abs(bundle_rows - want) / (1.0 + np.abs(want).max(axis=2, keepdims=True))
                cond = conditioning_many(want)
                assert (err.max(axis=(1, 2)) < STATE_TOL + 2e-14 * cond).all(), float(err.max())
    sel = np.nonzero(out["selectable"])[0]
    best500 = sel[np.argsort(out["cost"][sel], kind="stable")][:500]
    assert out["collision"][best500].mean() >= 0.25 and out["result"]["n_collisions"] > 500 and out["result"]["best_index"] >= 0


@pytest.mark.parametrize("lanes,mapping", [(1, 0), (2, 2), (4, 2), (2, 1)])
def test_many_ragged_obstacles(lanes, mapping):
    """40 obstacles (more than the hot table's one-step prefetch window of 25) whose predictions end at different steps:
    the masked obstacle loop, the dense fast path on the early steps and the lane-split fallback all against the oracle."""
    from oracle import oracle
    from frenetix_motion_planner_amd.problem import pack_predictions
    kw = dict(ref_kind="scurve", kappa=0.015, v0=9.0, grid=(6, 9, 11), n_obstacles=40, n_pred=30, lead_gap=40.0, seed=3,
              obstacle_min_gap=10.0)

    def build(hulls):
        inp = synthetic.make_inputs(hull_builder=hulls, **kw)
        preds = {}
        for j, (key, pr) in enumerate(inp.predictions.items()):
            n = 30 if j % 4 == 0 else (3 + (7 * j) % 27)           # some full length, the rest 3 .. 29 steps, one of 2
            if j == 5:
                n = 2                                                # <= 2 predicted steps: no hull at all
            preds[key] = dict(pos_list=pr["pos_list"][:n], cov_list=pr["cov_list"][:n], orientation_list=pr["orientation_list"][:n],
                              shape=pr["shape"])
        inp.obstacles = pack_predictions(preds, inp.n_samples, hulls)
        inp.predictions = preds
        return inp

    out = oracle.plan_step(build(oracle.build_obstacle_hulls))
    inp = build(hip_hulls())
    assert inp.obstacles["K"] == 40
    from frenetix_motion_planner_amd.engine import FrenetEngine
    with FrenetEngine(max_candidates=4096, max_obstacles=64, max_pred_steps=64) as e:
        e.set_tuning(lanes, 0, 2, 0, mapping)
        res = e.plan_step(inp)
        compare(e, inp, out, res)
        assert res["best_index"] == out["result"]["best_index"] and res["n_collisions"] == out["result"]["n_collisions"]
        assert out["collision"].sum() > 100 and out["result"]["n_collisions"] > 50 and res["best_index"] >= 0


def test_north_star_target_one_million_candidates():
    """BASELINE north star: >= 1 M candidate trajectories (30-step horizon, 20 obstacles) evaluated in < 10 ms on one
    MI355X -- every candidate checked against the oracle, the evaluation timed with HIP events."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    kw = dict(ref_kind="arc", v0=10.0, grid=(19, 230, 229), n_obstacles=20, n_pred=30, lead_gap=25.0, write_bundle=False,
              write_costmap=False)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    assert inp.n_candidates == 19 * 230 * 230 >= 1_000_000
    with FrenetEngine(max_candidates=inp.n_candidates + 64) as e:
        e.set_timing("kernel")
        res = e.plan_step(inp)
        cost, flags = e.costs()
        e.upload(inp)
        times = []
        for _ in range(5):
            e.evaluate()
            e.finish()
            times.append(e.last_kernel_ms)
    assert max(times) < 10.0, times
    ora = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
    f_ref, c_ref, best, best_cost = oracle.plan_range(ora, 0, ora.n_candidates, n_threads=min(32, len(__import__("os").sched_getaffinity(0))))
    sel = (f_ref & _abi.FX_FLAG_SELECTABLE) != 0
    differ = flags != f_ref
    assert differ.mean() < 1e-4
    settle_differing(ora, differ, flags, cost)      # every one of them: a last-ulp decision AND one of its admissible outcomes
    c = ((f_ref & _abi.FX_FLAG_COSTED) != 0) & ~differ
    assert (np.abs(cost[c] - c_ref[c]) / np.maximum(np.abs(c_ref[c]), 1e-12)).max() < COST_RTOL
    assert res["best_index"] == best and res["best_cost"] == pytest.approx(best_cost, rel=1e-9)
    assert ((f_ref & _abi.FX_FLAG_COLLISION) != 0)[sel].mean() > 0.25


def test_north_star_literal_bundle_and_obstacles_at_one_million_candidates():
    """The literal sentence of BASELINE's north star: >= 1 M candidates x 30 steps x 20 obstacles -- prediction cost, OBB collision
    check AND the SoA TrajectoryBundle in HBM -- in < 10 ms on one MI355X (measured ~0.9 ms).  Flags / costs / winner / collision
    count of every candidate against the oracle's range evaluation; the planes of every 64th costed candidate of a 1/64 sample
    (and of the winner) against the oracle at the fixed tolerance."""
    import os
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    from tests.admissible import conditioning_many
    kw = dict(ref_kind="arc", v0=10.0, grid=(19, 230, 229), n_obstacles=20, n_pred=30, lead_gap=25.0)   # = bench.py north_star
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    assert inp.n_candidates == 19 * 230 * 230 and inp.write_bundle and inp.collision
    ora = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
    with FrenetEngine(max_candidates=inp.n_candidates + 64) as e:
        e.set_timing("kernel")
        res = e.plan_step(inp)
        cost, flags = e.costs()
        info = e.step_info()
        assert info["lanes_per_candidate"] == 1 and not info["obstacle_kernel"]   # one fused kernel + the selection
        ids = np.arange(0, inp.n_candidates, 64 * 64)
        ids = np.unique(np.concatenate([ids, [res["best_index"]]]))
        rows = np.stack([e.sample(int(g)) for g in ids])
        e.upload(inp)
        times = []
        for _ in range(5):
            e.evaluate()
            e.finish()
            times.append(e.last_kernel_ms)
    assert max(times) < 10.0, times
    f_ref, c_ref, best, best_cost = oracle.plan_range(ora, 0, ora.n_candidates, n_threads=min(32, len(os.sched_getaffinity(0))))
    differ = flags != f_ref
    assert differ.mean() < 1e-4
    settle_differing(ora, differ, flags, cost)
    c = ((f_ref & _abi.FX_FLAG_COSTED) != 0) & ~differ
    assert (np.abs(cost[c] - c_ref[c]) / np.maximum(np.abs(c_ref[c]), 1e-12)).max() < COST_RTOL
    assert res["best_index"] == best and res["best_cost"] == pytest.approx(best_cost, rel=1e-9)
    sel = (f_ref & _abi.FX_FLAG_SELECTABLE) != 0
    coll = sel & ((f_ref & _abi.FX_FLAG_COLLISION) != 0)
    assert res["n_collisions"] == int(((c_ref[coll] < best_cost) | ((c_ref[coll] == best_cost) & (np.nonzero(coll)[0] < best))).sum())
    keep = [k for k, g in enumerate(ids) if (f_ref[g] & _abi.FX_FLAG_COSTED) and not differ[g]]
    assert len(keep) > 100
    want = np.stack([oracle.eval_forced(ora, int(ids[k]))["planes"] for k in keep])
    got = rows[keep]
    err = np.abs(got - want) / (1.0 + np.abs(want).max(axis=2, keepdims=True))
    assert (err.max(axis=(1, 2)) < STATE_TOL + 2e-14 * conditioning_many(want)).all(), float(err.max())


def _random_case(rng):
    kind = ["straight", "arc", "scurve"][int(rng.integers(3))]
    horizon = [2.0, 3.0, 5.0][int(rng.integers(3))]
    kw = dict(ref_kind=kind, kappa=float(rng.uniform(0.002, 0.03)) * (1 if rng.uniform() < 0.5 else -1) if kind != "scurve"
              else float(rng.uniform(0.005, 0.02)),
              n_knots=int(rng.integers(250, 600)), spacing=float(rng.uniform(0.4, 1.0)),
              v0=float([0.0, 0.5, 1.5, 4.0, 10.0, 22.0][int(rng.integers(6))]), a0=float(rng.uniform(-2, 2)),
              d0=float(np.round(rng.uniform(-1.5, 1.5), 2)), dd0=float(rng.uniform(-0.3, 0.3)), ddd0=float(rng.uniform(-0.3, 0.3)),
              horizon=horizon, v_des=float(rng.uniform(0, 20)), n_obstacles=int(rng.integers(0, 9)), n_pred=int(horizon / 0.1),
              draw_traj_set=bool(rng.integers(2)), kinematic_debug=bool(rng.integers(2)), seed=int(rng.integers(1 << 30)),
              lead_gap=float(rng.uniform(10, 40)) if rng.uniform() < 0.3 else 0.0)
    if rng.uniform() < 0.5:
        kw["level"] = int(rng.integers(0, 3))
    else:
        kw["grid"] = (int(rng.integers(1, 8)), int(rng.integers(1, 12)), int(rng.integers(1, 12)))
    if rng.uniform() < 0.15 and kw["v0"] > 1.0:
        kw["stop_point_s"] = float(rng.uniform(5, 40))
    if rng.uniform() < 0.2:
        kw["road_half_width"] = float(rng.uniform(2.5, 5.0))
    return kw


@pytest.mark.parametrize("case", range(32))
def test_random_scenarios_vs_oracle(case):
    """Seeded random scenarios (reference shape and curvature sign, standstill ... 22 m/s, horizons 2 / 3 / 5 s, sampling levels
    and dense grids down to a single candidate, 0-8 obstacles, debug flag sets, stop-point sampling, road boundary): every
    candidate of each against the oracle, under the automatic work decomposition."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    rng = np.random.default_rng([20241008, case])
    kw = _random_case(rng)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    with FrenetEngine(max_candidates=max(inp.n_candidates, 64), max_steps=inp.N, max_pred_steps=max(64, inp.N + 2)) as e:
        res = e.plan_step(inp)
        compare(e, inp, out, res)
        if np.all(out["margin"] >= FRAGILE):
            assert res["best_index"] == out["result"]["best_index"] and res["n_collisions"] == out["result"]["n_collisions"]
        if "road_half_width" in kw:
            bs = e.boundary_steps()
            walked = out["selectable"] & (out["margin"] >= FRAGILE)
            assert np.array_equal(bs[walked], out["boundary_step"][walked])


@pytest.mark.parametrize("horizon", [3.0, 10.0])
@pytest.mark.parametrize("lanes,mapping", [(0, 0), (1, 0), (2, 0)])
def test_maximum_obstacle_count_and_long_horizon(lanes, mapping, horizon):
    """The capacity edges of the obstacle stage: K = 64 obstacles (every bit of the per-step masks, bit 63 included) and a
    10 s horizon (N = 100 steps) -- against the oracle."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    # 10 s: the rows of a workgroup do not fit LDS -> generic kernel; 3 s: grid kernel with the staged hot table (64 x 80 B per wave)
    kw = dict(ref_kind="arc", kappa=0.008, n_knots=900, spacing=0.5, v0=3.0 if horizon > 5 else 9.0, horizon=horizon,
              grid=(9, 7, 9) if horizon > 5 else (7, 9, 21), n_obstacles=64, n_pred=int(horizon * 10), seed=11,
              obstacle_min_gap=45.0 if horizon > 5 else 14.0, v_des=4.0 if horizon > 5 else 10.0)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    assert inp.obstacles["K"] == 64 and inp.N == int(horizon * 10)
    with FrenetEngine(max_candidates=4096, max_steps=100, max_ref_knots=1024, max_obstacles=64, max_pred_steps=128) as e:
        e.set_tuning(lanes, 0, 0, 0, mapping)
        res = e.plan_step(inp)
        compare(e, inp, out, res)
        if np.all(out["margin"] >= FRAGILE):
            assert res["best_index"] == out["result"]["best_index"] and res["n_collisions"] == out["result"]["n_collisions"]
    assert out["collision"].sum() > 20 and out["result"]["n_feasible"] > 20


def test_update_state_equals_fresh_upload(eng):
    """fx_update_state (new ego state, sampling values and predictions rewritten in place, one small copy) gives bit for bit
    what a full upload of the same inputs gives -- flags, costs, planes, winner, counters."""
    kw = dict(ref_kind="arc", v0=10.0, grid=(7, 13, 13), n_obstacles=6, lead_gap=20.0)
    base = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    eng.plan_step(base)
    from frenetix_motion_planner_amd.problem import pack_predictions
    for j in range(3):
        moved = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
        moved.x0_lon = moved.x0_lon + np.array([0.4 * (j + 1), 0.1 * j, -0.05 * j])
        moved.x0_lat = moved.x0_lat + np.array([0.03 * (j + 1), 0.01, 0.0])
        moved.v_des = 11.0 + j
        moved.v_samp = moved.v_samp + 0.01 * (j + 1)
        preds = {k: dict(p, pos_list=np.asarray(p["pos_list"]) + 0.1 * (j + 1)) for k, p in moved.predictions.items()}
        moved.obstacles = pack_predictions(preds, moved.n_samples, hip_hulls())
        # in place
        eng.upload(base)
        up = eng.make_state_update(x0_lon=moved.x0_lon, x0_lat=moved.x0_lat, x0_orientation=moved.x0_orientation, v_des=moved.v_des,
                                   v_samp=moved.v_samp, obstacles=moved.obstacles)
        eng.update_state(up)
        eng.evaluate()
        ra = eng.finish()[0]
        ca, fa = eng.costs()
        pa = eng.bundle()
        # fresh
        rb = eng.plan_step(moved)
        cb, fb = eng.costs()
        pb = eng.bundle()
        assert np.array_equal(fa, fb) and np.array_equal(ca, cb) and np.array_equal(pa, pb)
        for k in ("best_index", "best_cost", "n_returned", "n_feasible", "n_collisions", "reason_hist"):
            assert ra[k] == rb[k], k
    # the combined call, state only (obstacles kept)
    eng.upload(base)
    up = eng.make_state_update(x0_lon=base.x0_lon + np.array([0.2, 0.0, 0.0]), v_des=12.5)
    r1 = eng.update_step_raw(up)[0]
    moved = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    moved.x0_lon = moved.x0_lon + np.array([0.2, 0.0, 0.0])
    moved.v_des = 12.5
    r2 = eng.plan_step(moved)
    assert r1.best_index == r2["best_index"] and r1.best_cost == r2["best_cost"] and r1.n_collisions == r2["n_collisions"]


def test_update_state_rejects_what_needs_a_new_upload(eng):
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), ref_kind="arc", v0=10.0, grid=(3, 5, 5))
    eng.plan_step(inp)
    with_obs = synthetic.make_inputs(hull_builder=hip_hulls(), ref_kind="arc", v0=10.0, grid=(3, 5, 5), n_obstacles=2)
    with pytest.raises(ValueError):
        eng.update_state(eng.make_state_update(obstacles=with_obs.obstacles))  # uploaded without obstacles
    # arrays of another shape than the upload's are refused before anything is read or rewritten (FxStateUpdate.nT .. P, ABI 8):
    # the library copies with the upload's counts out of the borrowed pointers
    eng.plan_step(with_obs)
    before = eng.plan_step(with_obs)
    with pytest.raises(ValueError):
        eng.update_state(eng.make_state_update(d_samp=np.linspace(-1.0, 1.0, len(with_obs.d_samp) - 1)))   # one lateral sample short
    with pytest.raises(ValueError):
        eng.update_state(eng.make_state_update(t_samp=np.concatenate([with_obs.t_samp, [2.9]])))
    three = synthetic.make_inputs(hull_builder=hip_hulls(), ref_kind="arc", v0=10.0, grid=(3, 5, 5), n_obstacles=3)
    with pytest.raises(ValueError):
        eng.update_state(eng.make_state_update(obstacles=three.obstacles))   # K = 3 arrays into a K = 2 upload
    short = synthetic.make_inputs(hull_builder=hip_hulls(), ref_kind="arc", v0=10.0, grid=(3, 5, 5), n_obstacles=2, n_pred=12)
    assert short.obstacles["P"] != with_obs.obstacles["P"]
    with pytest.raises(ValueError):
        eng.update_state(eng.make_state_update(obstacles=short.obstacles))   # another prediction stride P
    after = eng.step_raw()[0].as_dict()   # the refused updates left the resident step as it was
    assert all(after[k] == before[k] for k in ("best_index", "best_cost", "n_feasible", "n_returned", "n_collisions"))


@pytest.mark.gpu
def test_long_reference_runs_on_the_grid_kernel():
    """4 000 reference knots: the grid kernel keeps 8 B per knot in LDS (only the generic kernel stages the 64-byte records)"""
    from frenetix_motion_planner_amd.engine import FrenetEngine, build_obstacle_hulls
    from oracle import oracle
    inp = synthetic.make_inputs(ref_kind="arc", v0=9.0, grid=(5, 9, 11), n_obstacles=2, n_knots=4000, spacing=0.25, kappa=0.002,
                                hull_builder=build_obstacle_hulls)
    assert len(inp.coordinate_system.ref_pos) >= 3900
    with FrenetEngine(max_candidates=4096, max_ref_knots=4096) as eng:
        res = eng.plan_step(inp)
    ref = oracle.plan_step(inp, want_planes=False)["result"]
    assert res["best_index"] == ref["best_index"] and res["n_feasible"] == ref["n_feasible"]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [31, 32, 33, 48, 64])
@pytest.mark.parametrize("tuning", [(0, 0, 0, 0, 0), (1, 2, 1, 0, 0), (8, 2, 2, 128, 1), (2, 2, 2, 0, 1), (2, 2, 2, 0, 2)])
def test_thirty_two_and_more_obstacles_on_every_kernel_variant(K, tuning):
    """Obstacle 31 and beyond: the per-step masks are 64-bit words assembled from two 32-bit scalar reads -- a sign extension of
    the low half made obstacles 32 ... 63 appear on the generic kernel and the lane-split variants (found by the crowded soak:
    prediction cost inf).  Every kernel variant against the oracle, automatic decomposition included."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    kw = dict(ref_kind="arc", v0=9.0, grid=(3, 5, 7), n_obstacles=K, seed=K)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    with FrenetEngine(max_candidates=256, max_steps=inp.N, max_obstacles=64) as e:
        e.set_tuning(*tuning)
        res = e.plan_step(inp)
        compare(e, inp, out, res)
        assert res["n_collisions"] == out["result"]["n_collisions"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", [100211, 100666, 100833, 101349] + list(range(100000, 100012)))
def test_random_cost_functions_vs_oracle(case):
    """Random subsets of all ten cost terms with random weights over the random scenarios (the windowed terms run on the generic
    kernel).  The first four are the ones a 1 500-case soak flagged: standstill starts in LOW_VEL_MODE whose v alternates between
    +-1e6 m/s -- path_length, a signed sum, cancels to a few metres and agrees to what the v plane's tolerance allows
    (tests/admissible.py::signed_integral_slack), not to 1e-9 of the sum."""
    from frenetix_motion_planner_amd._abi import COST_NAMES
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    rng = np.random.default_rng([20241008, case])
    kw = _random_case(rng)
    # (lane_center_offset is drawn last, so that the cases above keep the draws that made the soak flag them)
    w = {n: float(rng.uniform(0.1, 5.0)) for n in COST_NAMES if n != "lane_center_offset" and rng.uniform() < 0.5}
    if rng.uniform() < 0.5:
        w["lane_center_offset"] = float(rng.uniform(0.1, 5.0))
        if rng.uniform() < 0.7:
            kw["lanelets"] = (float(rng.uniform(2.5, 4.5)), int(rng.integers(10, 120)))
    kw["cost_weights"] = w or {"lateral_jerk": 1.0}
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    with FrenetEngine(max_candidates=max(inp.n_candidates, 64), max_steps=inp.N, max_pred_steps=max(64, inp.N + 2)) as e:
        res = e.plan_step(inp)
        compare(e, inp, out, res)
        if np.all(out["margin"] >= FRAGILE):
            assert res["best_index"] == out["result"]["best_index"] and res["n_collisions"] == out["result"]["n_collisions"]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [65, 100, 128, 129, 200, 256])
@pytest.mark.parametrize("tuning", [(0, 0, 0), (1, 2, 1), (2, 3, 1), (8, 2, 1), (32, 2, 1)])
def test_more_than_sixty_four_obstacles(K, tuning):
    """65 ... 256 predicted obstacles (FX_MAX_OBSTACLES): the per-step masks take one 64-bit word per 64 obstacles and the step
    runs on the generic kernel -- one lane per candidate and split horizons, ranges and (K = 100) a sampling matrix -- against
    the oracle; the reference itself has no obstacle limit."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    kw = dict(ref_kind="arc", v0=9.0, grid=(3, 5, 7), n_obstacles=K, seed=K, as_matrix=(K == 100))
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    out = oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw))
    with FrenetEngine(max_candidates=256, max_steps=inp.N, max_obstacles=256) as e:
        e.set_tuning(*tuning)
        res = e.plan_step(inp)
        assert not e.step_info()["grid_kernel"]
        compare(e, inp, out, res)
        assert res["n_collisions"] == out["result"]["n_collisions"]
        # the in-place state update rebuilds the multi-word tables too
        res2 = e.plan_step(inp)
        assert res2["best_index"] == res["best_index"] and res2["best_cost"] == res["best_cost"]


@pytest.mark.gpu
def test_winner_decided_by_a_last_ulp_cost_tie_is_an_admissible_outcome():
    """Soak case 2170242 (round 6, tools/soak_batch.py), agent 1: the lateral grid holds -1.2000000000000002 and the appended current
    offset -1.2 -- two candidates (519, 527) whose total costs are the SAME double in the oracle's arithmetic and one ulp apart in
    the lane-split kernel's (its sums over the horizon are trees, the reference's are sequential).  The stable (cost, index) arg-min
    then answers 519 on one side and 527 on the other.  What is held: every other field by compare(), the two winners' reference
    costs within 8 ulp, the device's own winner = arg-min of the device's own costs with the index as tie-break."""
    from frenetix_motion_planner_amd import _abi
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    rng = np.random.default_rng([20241008, 2170242])
    kws = [_random_case(rng) for _ in range(int(rng.integers(2, 6)))]
    for kw in kws:
        kw.pop("stop_point_s", None) if rng.uniform() < 0.5 else None
    inps = [synthetic.make_inputs(hull_builder=hip_hulls(), **kw) for kw in kws]
    outs = [oracle.plan_step(synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)) for kw in kws]
    assert -1.2 in inps[1].d_samp and np.count_nonzero(np.abs(np.asarray(inps[1].d_samp) + 1.2) < 1e-12) == 2
    cap = sum(max(i.n_candidates, 64) + 64 for i in inps)
    with FrenetEngine(max_candidates=cap, max_steps=max(i.N for i in inps), max_pred_steps=64, max_obstacles=256, max_agents=len(inps)) as e:
        res = e.plan_batch(inps)
        for a, (inp, out) in enumerate(zip(inps, outs)):
            compare(e, inp, out, res[a], agent=a)
            assert bool(np.all(out["margin"] >= FRAGILE))
            ga, gb = res[a]["best_index"], out["result"]["best_index"]
            if gb < 0:   # (an agent of the batch without a survivor)
                assert ga == gb
                continue
            assert ga >= 0 and abs(out["cost"][ga] - out["cost"][gb]) <= 8 * np.spacing(abs(out["cost"][gb]))
            if a != 1:
                assert ga == gb and res[a]["n_collisions"] == out["result"]["n_collisions"]
            cost, flags = e.costs(a)
            ok = ((flags & _abi.FX_FLAG_SELECTABLE) != 0) & ((flags & (_abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY)) == 0) & ~np.isnan(cost)
            ids = np.nonzero(ok)[0]
            assert ga == int(ids[np.lexsort((ids, cost[ids]))][0]) and res[a]["best_cost"] == cost[ga]
        assert {res[1]["best_index"], outs[1]["result"]["best_index"]} <= {519, 527}
        assert outs[1]["cost"][519] == outs[1]["cost"][527]


@pytest.mark.gpu
def test_obstacle_limit_is_reported():
    from frenetix_motion_planner_amd.problem import MAX_OBSTACLES
    with pytest.raises(ValueError, match="at most"):
        synthetic.make_inputs(hull_builder=hip_hulls(), ref_kind="arc", v0=9.0, grid=(1, 2, 2), n_obstacles=MAX_OBSTACLES + 1)


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("what", ["s0", "v0", "a0", "d0", "dd0", "obstacle_pos", "cov_inv", "hull", "v_des"])
def test_non_finite_inputs(what):
    """NaN / inf in the ego state, the predictions or the desired velocity (an upstream fault; the reference has no test for
    it): the step completes, the masks equal the oracle's wherever the ego state is finite, and a candidate whose cost is
    NaN is never selected -- the reference's sort would leave such candidates in list order and take the first."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    from oracle import oracle
    kw = dict(ref_kind="arc", v0=9.0, grid=(3, 5, 7), n_obstacles=3)
    inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
    ref = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
    for x in (inp, ref):
        if what in ("s0", "v0", "a0"):
            x.x0_lon = np.array(x.x0_lon, dtype=np.float64)
            x.x0_lon[("s0", "v0", "a0").index(what)] = np.inf if what == "a0" else np.nan
        elif what in ("d0", "dd0"):
            x.x0_lat = np.array(x.x0_lat, dtype=np.float64)
            x.x0_lat[("d0", "dd0").index(what)] = np.inf if what == "dd0" else np.nan
        elif what == "obstacle_pos":
            x.obstacles["pos"] = np.array(x.obstacles["pos"]); x.obstacles["pos"][0, 3] = np.nan
        elif what == "cov_inv":
            x.obstacles["cov_inv"] = np.array(x.obstacles["cov_inv"]); x.obstacles["cov_inv"][1, 2] = np.inf
        elif what == "hull":
            x.obstacles["hull"] = np.array(x.obstacles["hull"]); x.obstacles["hull"][2, 4, 0] = np.nan
        else:
            x.v_des = np.nan
    out = oracle.plan_step(ref)
    with FrenetEngine(max_candidates=256, max_steps=inp.N) as e:
        res = e.plan_step(inp)
        cost, flags = e.costs()
    if what in ("s0", "v0", "a0", "d0", "dd0"):
        assert res["best_index"] == -1 == out["result"]["best_index"] and res["n_feasible"] == 0 == out["result"]["n_feasible"]
    else:
        assert np.array_equal(flags, out["flags"])
        assert res["n_feasible"] == out["result"]["n_feasible"] and res["n_collisions"] == out["result"]["n_collisions"]
        costed = (flags & _abi.FX_FLAG_COSTED) != 0
        if np.isnan(cost[costed]).all():
            assert res["best_index"] == -1
        else:
            assert res["best_index"] == out["result"]["best_index"]


def test_topk_random_sizes_against_numpy():
    """Top-k survivors (one-wave slice kernel with register-resident entries, head-pointer merge; the general kernels beyond
    their sizes) against a NumPy lexicographic sort of the eligible candidates: ragged sizes, ties, k = 1 ... 64."""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    rng = np.random.default_rng(7)
    for case in range(24):
        grid = (int(rng.integers(1, 12)), int(rng.integers(1, 30)), int(rng.integers(1, 30)))
        inp = synthetic.make_inputs(hull_builder=hip_hulls(), ref_kind="arc", v0=float(rng.uniform(1, 15)), grid=grid,
                                    n_obstacles=int(rng.integers(0, 6)), seed=case,
                                    cost_weights=({"velocity_offset": 1.0} if case % 3 == 0 else None))   # few distinct costs: ties
        with FrenetEngine(max_candidates=inp.n_candidates + 64) as e:
            e.plan_step(inp)
            cost, flags = e.costs()
            el = np.nonzero(((flags & _abi.FX_FLAG_SELECTABLE) != 0) & ((flags & (_abi.FX_FLAG_COLLISION | _abi.FX_FLAG_BOUNDARY)) == 0)
                            & ~np.isnan(cost))[0]
            order = el[np.lexsort((el, cost[el]))]
            for k in (1, 5, 32, 64):
                c, i = e.topk(k)
                want = list(order[:k]) + [-1] * (k - min(k, len(order)))
                assert list(i[0]) == want, (case, k, grid)
                assert np.array_equal(c[0][:len(order[:k])], cost[order[:k]])
