"""The references and input sets of tests/test_device_math.py, held on the CPU: each reference against an independent one where
one exists, each input set against its coverage conditions (no GPU needed)."""
import json
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from tests import device_math_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
MEASURED_JSON = os.path.join(ROOT, "profiles", "device_math", "measured.json")


def _sample(x, n, seed):
    return x[np.random.default_rng(seed).choice(x.size, n, replace=False)]


# ---- the number formats ------------------------------------------------------------------------------------------------------
def test_longdouble_is_the_64_bit_significand_format_and_agrees_with_mpmath():
    """the bulk reference of atan / sin / cos / 1/sqrt is np.longdouble: 2^-11 double-ulp if it is x87 extended and its libm is
    good -- both asserted: 2 000 sampled points of the device's input sets, zeros of sin and cos included, within 2^-9 double-ulp"""
    assert np.finfo(LD).nmant == 63
    assert mpmath.__version__ == "1.3.0"
    xa = R.atan_inputs().x[0]
    xa = _sample(xa[np.isfinite(xa)], 2_000, 1)
    I = R.sincos_inputs()
    xs = np.concatenate([I.x[0][I.seg["k_pi_2"]][::2], _sample(I.x[0], 1_400, 2)])   # ~600 points next to zeros of sin or cos
    assert xs.size >= 2_000
    tol = 2.0 ** -9
    with mpmath.workprec(R.MP_PREC):
        for fn_ld, fn_mp, x in ((np.arctan, mpmath.atan, xa), (np.sin, mpmath.sin, xs), (np.cos, mpmath.cos, xs)):
            got = fn_ld(x.astype(LD))
            worst = 0.0
            for v, g in zip(x, got):
                r = fn_mp(mpmath.mpf(float(v)))
                u = np.spacing(abs(float(r))) if float(r) != 0 else 5e-324
                worst = max(worst, float(abs(R.mp_of_ld(g) - r) / mpmath.mpf(u)))
            assert worst <= tol, (fn_mp.__name__, worst)
        xq = _sample(R.divisor_inputs(False).x[0], 2_000, 3)
        got = LD(1) / np.sqrt(xq.astype(LD))
        for v, g in zip(xq, got):
            r = 1 / mpmath.sqrt(mpmath.mpf(float(v)))
            assert abs(R.mp_of_ld(g) - r) / r <= tol * 2.0 ** -53


def test_mpmath_agrees_with_numpy_within_one_ulp():
    xa = R.atan_inputs().x[0]
    xa = _sample(xa[np.isfinite(xa)], 1_500, 4)
    xs = _sample(R.sincos_inputs().x[0], 1_500, 5)
    xs = xs[(np.abs(np.sin(xs)) > 1e-3) & (np.abs(np.cos(xs)) > 1e-3)]
    assert R.mp_err(np.arctan(xa), R.mp_atan(xa)).max() <= 1.0
    assert R.mp_err(np.sin(xs), R.mp_sin(xs)).max() <= 1.0
    assert R.mp_err(np.cos(xs), R.mp_cos(xs)).max() <= 1.0
    xq = _sample(R.divisor_inputs(False).x[0], 1_000, 6)
    assert R.mp_err(np.sqrt(xq), R.mp_unary(mpmath.sqrt, xq)).max() <= 0.5     # np.sqrt is correctly rounded
    assert R.mp_err(1.0 / np.sqrt(xq), R.mp_rsqrt(xq)).max() <= 1.5


def test_fraction_division_is_ieee_division():
    I = R.quotient_inputs()
    a, b = I.x
    idx = np.random.default_rng(7).choice(a.size, 3_000, replace=False)
    for i in idx:
        rn, q = R.frac_div(a[i], b[i])
        assert rn == a[i] / b[i]
        assert abs(Fraction(float(rn)) - q) <= Fraction(float(np.spacing(abs(rn)))) / 2
    # the error measure: the correctly rounded quotient is within half an ulp, its neighbour between half and one and a half
    a, b = a[idx], b[idx]
    rn = a / b
    assert R.frac_div_err(rn, a, b).max() <= 0.5
    up = R.frac_div_err(np.nextafter(rn, np.inf), a, b)
    assert up.min() >= 0.5 and up.max() <= 1.5
    rep = R.div_report(np.where(np.arange(rn.size) % 100 == 0, np.nextafter(rn, np.inf), rn), a, b)
    assert rep["n_unequal"] == 30 and 0.5 <= rep["max_ulp"] <= 1.5
    # Markstein's exception is in the set: an all-ones mantissa
    d = R.divisor_inputs(True).x[0]
    assert float.fromhex("0x1.fffffffffffffp+0") in d and 1.0 in d


def test_np_round_is_rint_of_the_scaled_value_over_the_scale():
    """np.round(x, 5) is the planner's own operation; what it computes -- rint(x * 1e5) / 1e5 -- is what np_round5 restates"""
    x = R.round5_inputs().x[0]
    assert R.bits_equal(np.round(x, 5), np.rint(x * 1e5) / 1e5).all()


def test_wrap_reference_is_the_scalar_loop():
    a = R.wrap_inputs().x[0]
    ref = R.np_wrap_pm_2pi(a)
    for v, r in zip(a[:2_000], ref[:2_000]):
        v = float(v)
        while v > R.TWO_PI:
            v -= R.TWO_PI
        while v < -R.TWO_PI:
            v += R.TWO_PI
        assert v == r and np.signbit(v) == np.signbit(r)
    with pytest.raises(AssertionError):
        R.np_wrap_pm_2pi(np.array([np.inf]))


# ---- the hull ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hull():
    I = R.hull_inputs()
    in0, in1, in2 = I.x
    return I, in0, in1, in2, R.hull_scale(in0, in1, in2), R.ld_hull(in0, in1, in2), R.oracle_hull(in0, in1, in2)


def oracle_hull_figures(I, in0, in1, in2, scale, ref, orc):
    e = R.hull_err_ld(orc, ref, scale)
    ns = I.seg["random"].start
    e[:ns] = R.hull_err_mp(orc[:ns], R.mp_hull(in0[:ns], in1[:ns], in2[:ns]), scale[:ns])
    return {"centre": float(e[:, 0:2].max()), "axis": float(e[:, 2:4].max()), "extents": float(e[:, 4:6].max())}


def test_longdouble_hull_is_the_mpmath_hull(hull):
    I, in0, in1, in2, scale, ref, _ = hull
    ns = I.seg["random"].start
    idx = np.concatenate([np.arange(ns), ns + np.random.default_rng(8).choice(in0.shape[0] - ns, 600, replace=False)])
    mref = R.mp_hull(in0[idx], in1[idx], in2[idx])
    with mpmath.workprec(R.MP_PREC):
        one = mpmath.mpf(np.spacing(1.0))
        for j, i in enumerate(idx):
            for k in range(6):
                u = one if k in (2, 3) else mpmath.mpf(float(scale[i]))
                assert abs(R.mp_of_ld(ref[i, k]) - mref[j][k]) / u <= 2.0 ** -3, (I.name_of(i), k)
    # (2^-3 of the unit, where the device's bound is >= 2 units: the centre is recomposed from projections of coordinates up to
    # 300 m -- 2^6 ulps of the scale -- in a format of 2^-11 double-ulp, over a handful of operations)
    for name in ("pi-1e-13", "opposite"):     # |u0 + u1| < 1e-12: the first box's axis
        s = I.seg[name]
        assert np.array_equal(ref[s, 2:4].astype(np.float64), in0[s, 2:4])
        assert all(float(m[2]) == in0[i, 2] and float(m[3]) == in0[i, 3] for m, i in zip(mref[s.start:s.stop], range(s.start, s.stop)))


def test_hull_reference_against_the_oracle_within_the_measured_figure(hull):
    """the oracle's own error against the exact hull: it sets the device's bound (twice it, at least 2 ulp), is recorded in
    profiles/device_math/measured.json and must not have grown past the recorded figure (its inputs go through this machine's
    cos / sin, hence the quarter of slack)"""
    fig = oracle_hull_figures(*hull)
    print("\n[device_math] oracle obb_hull, ulps:", fig)
    rec = json.load(open(MEASURED_JSON))["oracle_obb_hull"]
    for k, v in fig.items():
        assert v <= 1.25 * rec[k] and v >= 0.5 * rec[k], (k, v, rec[k])
    assert fig["axis"] <= 1.5      # the oracle normalises with sqrt and a division


def test_hull_inputs_cover_what_they_should(hull):
    I, in0, in1, in2, *_ = hull
    assert in0.shape[0] <= 300_000 and I.seg["random"].stop - I.seg["random"].start == 20_000
    assert np.abs(np.concatenate([in0[:, :2], in1[:, :2]])).max() <= 300.0
    sep = np.hypot(in1[:, 0] - in0[:, 0], in1[:, 1] - in0[:, 1])
    assert sep.max() <= 5.0 + 1e-9 and sep.min() == 0.0
    assert {tuple(r) for r in in2} == {R.CAR, R.TRUCK}
    for M in (in0, in1):
        assert np.abs(np.hypot(M[:, 2], M[:, 3]) - 1.0).max() < 4e-16
    mn = np.hypot(in0[:, 2] + in1[:, 2], in0[:, 3] + in1[:, 3])
    assert np.all(mn[I.seg["opposite"]] == 0.0) and np.all(mn[I.seg["pi-1e-13"]] < 1e-12) and np.all(mn[I.seg["pi-1e-13"]] > 0)
    assert np.all(mn[I.seg["pi-1e-6"]] > 1e-12) and np.all(mn[I.seg["equal"]] > 1.99)
    rnd = I.seg["random"]
    assert (np.abs(mn[rnd] - 1e-12) > 1e-13).all()      # no random pair sits on the switch


# ---- the overlap test ----------------------------------------------------------------------------------------------------------
def test_overlap_reference_and_inputs():
    from oracle import oracle
    import ctypes as C
    I = R.overlap_inputs()
    A, B = I.x
    assert A.shape[0] <= 300_000 and I.seg["random"].stop - I.seg["random"].start == 20_000
    dec, tight = R.overlap_reference(A, B)
    # the triage by np.longdouble decides as Fraction does
    idx = np.concatenate([np.arange(I.seg["random"].start), I.seg["random"].start + np.arange(1_500)])
    dx, tx = R.overlap_reference(A[idx], B[idx], exact_all=True)
    assert np.array_equal(dx, dec[idx]) and np.abs(tx - tight[idx]).max() < 1e-12
    for name in ("touch_edge", "touch_corner"):
        s = I.seg[name]
        assert dec[s].all() and np.all(tight[s] == 0.0)       # touching collides, exactly
        assert np.all(A[s] == np.rint(A[s])) and np.all(B[s] == np.rint(B[s]))
    for name in ("inside", "inside_rotated", "rotated_in_2^-20"):
        assert dec[I.seg[name]].all()
    for name in ("apart_2^-20", "rotated_apart_2^-20"):
        s = I.seg[name]
        assert not dec[s].any() and np.abs(tight[s] - 2.0 ** -20).max() < 1e-12
    rnd = I.seg["random"]
    assert (tight[rnd] <= 1e-9).mean() <= 0.01 and 0.2 < dec[rnd].mean() < 0.8
    # the oracle's double test agrees wherever the decision is not within 1e-9 of flipping
    L = oracle.lib()
    pd = C.POINTER(C.c_double)
    L.fxo_obb_overlap.argtypes, L.fxo_obb_overlap.restype = [pd, pd], C.c_int32
    Ac, Bc = np.ascontiguousarray(A), np.ascontiguousarray(B)
    for i in np.flatnonzero(tight > 1e-9)[::7]:
        assert bool(L.fxo_obb_overlap(Ac[i].ctypes.data_as(pd), Bc[i].ctypes.data_as(pd))) == dec[i], I.name_of(i)


# ---- the other input sets ----------------------------------------------------------------------------------------------------
def test_atan_inputs_reach_every_interval():
    I = R.atan_inputs()
    x = I.x[0]
    assert x.size <= 300_000
    counts = np.bincount(R.atan_interval(x)[~np.isnan(x)], minlength=5)
    assert counts.min() >= 5_000, counts
    for e in R.ATAN_EDGES:
        for v in (e, np.nextafter(e, 0), np.nextafter(e, 9), -e, -np.nextafter(e, 0), -np.nextafter(e, 9)):
            assert v in x[I.seg["edges"]]
    sp = x[I.seg["special"]]
    assert np.isnan(sp).sum() == 1 and np.inf in sp and -np.inf in sp and 2.0 ** -27 in sp and 5e-324 in sp and 1e300 in sp and 1e-300 in sp
    assert np.signbit(sp[sp == 0]).tolist() == [False, True]
    assert (np.abs(x) < 0.4375).sum() >= 50_000


def test_sincos_inputs_reach_every_quadrant_with_both_signs():
    I = R.sincos_inputs()
    x = I.x[0]
    assert x.size <= 300_000 and np.isfinite(x).all() and np.abs(x).max() <= 1e6
    q, neg = R.sincos_quadrant(x)
    for k in range(4):
        assert ((q == k) & neg).sum() >= 10_000 and ((q == k) & ~neg).sum() >= 10_000
    kp = x[I.seg["k_pi_2"]]
    assert kp.size == 3 * 401 and (np.abs(x) <= 64).sum() >= 100_000


def test_divisor_and_quotient_inputs():
    for signed in (True, False):
        I = R.divisor_inputs(signed)
        d = I.x[0]
        assert d.size <= 300_000 and np.isfinite(d).all() and (np.abs(d) >= np.finfo(np.float64).tiny).all()
        assert signed == bool((d < 0).any())
        assert (d[I.seg["below2"]] < 2).all() and (d[I.seg["below2"]] > 1.9999999).all() and np.unique(d[I.seg["below2"]]).size == 2_000
        assert d[I.seg["above1"]][0] == 1.0 and np.unique(d[I.seg["above1"]]).size == 2_000
        ex = np.frexp(d[I.seg["random"]])[1] - 1
        assert ex.min() == -40 and ex.max() == 39
    ko = R.kernel_operands()
    T = np.arange(1, 101) * 0.1
    for v in (T[6] ** 2, (T[6] * T[6]) * T[6], 3.0 * (T[99] * T[99]), 1.0, 0.1):
        assert v in ko
    assert ko.min() >= 1e-5 and ko.max() <= 1e5 + 1
    I = R.quotient_inputs()
    a, b = I.x
    assert a.size <= 300_000 and (b != 0).all() and np.isfinite(a).all() and np.isfinite(b).all()


def test_round5_and_wrap_inputs():
    I = R.round5_inputs()
    x = I.x[0]
    k = np.array([-200_000, -1, 0, 1, 12_345, 200_000])
    t = x[I.seg["ties"]]
    for v in k * 1e-5 + 5e-6:
        assert v in t and np.nextafter(v, 9) in t and np.nextafter(v, -9) in t
    assert t.size == 3 * 400_001 and np.abs(x[I.seg["yaw"]]).max() <= 10
    lg = np.abs(x[I.seg["loguniform"]])
    assert lg.min() >= 1e-12 and lg.max() <= 1e9 and lg.min() < 1e-11 and lg.max() > 1e8
    a = R.wrap_inputs().x[0]
    assert a.size <= 300_000 and np.isfinite(a).all() and np.abs(a).max() <= R.WRAP_MAX
    for v in (R.TWO_PI, np.nextafter(R.TWO_PI, 9), np.nextafter(R.TWO_PI, 0), -R.TWO_PI, 0.0, 40 * (np.pi / 2), -40 * (np.pi / 2)):
        assert v in a


# ---- the entry point, without a device -----------------------------------------------------------------------------------------
def test_selftest_ops_match_the_header_and_bad_calls_are_refused_before_any_launch():
    from frenetix_motion_planner_amd import engine
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"FX_SELFTEST_([A-Z0-9_]+) = (\d+)", hdr)}
    assert codes.pop("n_ops") == len(engine.SELFTEST_OPS) == 15
    assert codes == {k: v[0] for k, v in engine.SELFTEST_OPS.items()}
    assert float(re.search(r"#define FX_SELFTEST_WRAP_MAX ([0-9.]+)", hdr).group(1)) == R.WRAP_MAX
    # nothing below reaches a device: the checks come first (a shared GPU must never see wrap_pm_2pi's endless loop)
    for bad in (np.inf, -np.inf, np.nan, 1e300, np.nextafter(R.WRAP_MAX, 1e9)):
        with pytest.raises(ValueError, match="wrap_pm_2pi"):
            engine.device_selftest("wrap_pm_2pi", np.array([0.0, bad]))
    with pytest.raises(ValueError, match="outside"):
        engine.device_selftest("atan", np.zeros(0))
    with pytest.raises(ValueError):
        engine.device_selftest("fdiv", np.zeros(3), np.zeros(4))
    with pytest.raises(ValueError):
        engine.device_selftest("obb_hull", np.zeros((3, 4)), np.zeros((3, 4)))


def test_measured_file_holds_what_the_design_table_quotes():
    m = json.load(open(MEASURED_JSON))
    assert re.fullmatch(r"[0-9a-f]{7,40}", m["device_kernels_of_commit"])
    assert set(m["oracle_obb_hull"]) == {"centre", "axis", "extents"}
    dev = m["device"]
    assert set(dev) == set(__import__("frenetix_motion_planner_amd.engine", fromlist=["x"]).SELFTEST_OPS)
    assert dev["atan"]["max_ulp"] <= 1.0 and dev["rcp_pred"]["max_ulp"] <= 11.0 and dev["sqrt_rsqrt"]["rsq_max_rel"] <= 2.0 ** -51
    assert max(dev["sincos"]["max_abs_64"], dev["sincos"]["max_abs_1e6"]) < 4e-16
    for k in ("centre", "axis", "extents"):
        assert dev["obb_hull"][k]["device_max"] <= dev["obb_hull"][k]["bound"]
