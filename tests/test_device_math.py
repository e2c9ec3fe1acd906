"""Every device arithmetic primitive (csrc/fx_math.h, fx_walk.h, fx_eval_kernel.h) against an exact reference, on a real MI355X.

fx_device_selftest runs ONE primitive of the product headers elementwise (csrc/fx_selftest_kernel.h); the references and the input
sets are tests/device_math_ref.py (held themselves by tests/test_device_math_ref.py, no GPU).  Every test prints its figures
before it asserts; the last one prints the table of DESIGN.md section 2 ("The device primitives") and, with
FXPLAN_RECORD_MEASURED=<file>, writes it there (profiles/device_math/measured.json is such a file: a run of the suite itself
rewrites no tracked file).
"""
import json
import os

import numpy as np
import pytest

from tests import device_math_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = {}
_CACHE = {}
LD = np.longdouble


def dev(op, *arrays):
    from frenetix_motion_planner_amd.engine import device_selftest
    return device_selftest(op, *arrays)


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def same_bits(a, b):
    """bit-identical, NaN results counting as equal to each other"""
    return R.bits_equal(a, b) | (np.isnan(a) & np.isnan(b))


def worst(I, err, cols=None, k=3):
    """the k worst points of an input set, named"""
    order = np.argsort(-np.nan_to_num(err, nan=np.inf))[:k]
    xs = I.x if cols is None else cols
    return "; ".join(f"{I.name_of(i)} x={[float(c[i]) if c.ndim == 1 else c[i].tolist() for c in xs]} err={err[i]:.4g}" for i in order)


def record(op, **kw):
    MEASURED.setdefault(op, {}).update({k: (float(v) if isinstance(v, (np.floating, float)) else int(v) if isinstance(v, (np.integer, int)) else v)
                                        for k, v in kw.items()})
    print(f"\n[device_math] {op}: " + ", ".join(f"{k} = {MEASURED[op][k]}" for k in kw))


# ---------------------------------------------------------------------------------------------------------------------------
# atan
# ---------------------------------------------------------------------------------------------------------------------------
def _atan():
    I = R.atan_inputs()
    x = I.x[0]
    return I, x, dev("atan", x)[0]


def test_atan_within_one_ulp_of_the_true_value():
    I, x, got = cached("atan", _atan)
    fin = np.isfinite(x)
    err = np.zeros(x.size)
    with np.errstate(all="ignore"):
        err[fin] = R.ulp_err_ld(got[fin], np.arctan(x[fin].astype(LD))).astype(np.float64)
    ns = I.seg["uniform64"].start               # the structured points: mpmath
    st = np.flatnonzero(fin[:ns])
    err[st] = R.mp_err(got[st], R.mp_atan(x[st]))
    by_interval = [float(err[fin & (R.atan_interval(x) == k)].max()) for k in range(5)]
    record("atan", n=x.size, max_ulp=err.max(), max_ulp_by_interval=by_interval)
    assert err.max() <= 1.0, worst(I, err)
    sp = I.seg["special"]
    xs, gs = x[sp], got[sp]
    assert gs[1] == 0 and np.signbit(gs[1]) and gs[0] == 0 and not np.signbit(gs[0])   # atan(-0) = -0, atan(+0) = +0
    pio2 = np.float64(np.pi / 2)
    assert gs[xs == np.inf][0] == pio2 and gs[xs == -np.inf][0] == -pio2, gs
    assert np.isnan(gs[np.isnan(xs)]).all()
    tiny = np.abs(xs) <= 2.0 ** -27             # atan(x) = x to the last bit
    assert np.array_equal(gs[tiny], xs[tiny])


def test_atan_table_variant_is_bit_identical():
    I, x, got = cached("atan", _atan)
    tab = dev("atan_tab", x)[0]
    ne = np.flatnonzero(~same_bits(tab, got))
    record("atan_tab", n=x.size, n_not_identical=ne.size)
    assert ne.size == 0, [(I.name_of(i), x[i], got[i], tab[i]) for i in ne[:5]]


@pytest.mark.parametrize("op", ["atan_small", "atan_small_tab"])
def test_atan_small_variants_are_bit_identical_below_7_16(op):
    """Measured on the MI355X: bit-identical to atan<false> on all 109 406 inputs below 7/16 that are not -0.  The one exception
    is x = -0: x - x * p(x) is -0 - (-0) = +0 where atan's copysign gives -0 (value-equal; theta_cl + theta_ref does not see it)."""
    I, x, got = cached("atan", _atan)
    m = np.abs(x) < 0.4375
    assert m.sum() >= 100_000
    xs, ref = x[m], got[m]
    small = dev(op, xs)[0]
    ne = np.flatnonzero(~same_bits(small, ref))
    record(op, n=int(m.sum()), n_not_identical=ne.size, not_identical_inputs=[float(v).hex() for v in xs[ne][:8]])
    neg0 = (xs == 0) & np.signbit(xs)
    assert neg0.sum() == 1 and np.all(small[neg0] == 0) and not np.signbit(small[neg0]).any()   # the exception, held as it is
    assert not (ne.size and (~neg0[ne]).any()), [(xs[i], ref[i], small[i]) for i in ne[~neg0[ne]][:5]]


# ---------------------------------------------------------------------------------------------------------------------------
# sin / cos
# ---------------------------------------------------------------------------------------------------------------------------
def _sincos():
    I = R.sincos_inputs()
    x = I.x[0]
    sn, cs = dev("sincos", x)
    xl = x.astype(LD)
    ref_s, ref_c = np.sin(xl), np.cos(xl)
    abs_s, abs_c = np.abs(sn.astype(LD) - ref_s).astype(np.float64), np.abs(cs.astype(LD) - ref_c).astype(np.float64)
    ns = I.seg["uniform64"].start               # structured: multiples of pi/2 with their neighbours, +-0 -- mpmath
    st = np.arange(ns)
    mps, mpc = R.mp_sin(x[st]), R.mp_cos(x[st])
    abs_s[st], abs_c[st] = R.mp_err(sn[st], mps, unit=1.0), R.mp_err(cs[st], mpc, unit=1.0)
    rel_zero = max(R.mp_err(sn[st], mps).max(), R.mp_err(cs[st], mpc).max())   # in ulps of the value, next to the zeros
    return dict(I=I, x=x, sn=sn, cs=cs, ref_s=ref_s, ref_c=ref_c, abs_s=abs_s, abs_c=abs_c, rel_zero=rel_zero)


def test_sincos_on_the_kernels_range():
    d = cached("sincos", _sincos)
    I, x = d["I"], d["x"]
    m = np.abs(x) <= 64
    mid = m & (np.abs(d["ref_s"]) > 0.1) & (np.abs(d["ref_c"]) > 0.1)
    us, uc = R.ulp_err_ld(d["sn"][mid], d["ref_s"][mid]).astype(np.float64), R.ulp_err_ld(d["cs"][mid], d["ref_c"][mid]).astype(np.float64)
    record("sincos", n_64=int(m.sum()), max_abs_64=max(d["abs_s"][m].max(), d["abs_c"][m].max()), max_ulp_away_from_zeros=max(us.max(), uc.max()),
           max_ulp_next_to_zeros=d["rel_zero"])
    assert d["abs_s"][m].max() < 4e-16, worst(I, np.where(m, d["abs_s"], 0))
    assert d["abs_c"][m].max() < 4e-16, worst(I, np.where(m, d["abs_c"], 0))
    assert us.max() <= 2.0 and uc.max() <= 2.0, (us.max(), uc.max())
    z = I.seg["zero"]   # sin(+-0) = +0 (the reduction's fma(-n, pi/2, x) is +0 + -0), cos = 1
    assert np.all(d["sn"][z] == 0.0) and not np.signbit(d["sn"][z]).any() and np.all(d["cs"][z] == 1.0)


def test_sincos_on_the_claimed_range():
    """fx_math.h: "for |x| up to ~1e6" -- the same absolute bound there"""
    d = cached("sincos", _sincos)
    record("sincos", n_1e6=d["x"].size, max_abs_1e6=max(d["abs_s"].max(), d["abs_c"].max()))
    assert d["abs_s"].max() < 4e-16, worst(d["I"], d["abs_s"])
    assert d["abs_c"].max() < 4e-16, worst(d["I"], d["abs_c"])


def test_sincos_table_variant_is_bit_identical():
    d = cached("sincos", _sincos)
    sn, cs = dev("sincos_tab", d["x"])
    ne = np.flatnonzero(~(same_bits(sn, d["sn"]) & same_bits(cs, d["cs"])))
    record("sincos_tab", n=d["x"].size, n_not_identical=ne.size)
    assert ne.size == 0, [(d["I"].name_of(i), d["x"][i], d["sn"][i], sn[i], d["cs"][i], cs[i]) for i in ne[:5]]


# ---------------------------------------------------------------------------------------------------------------------------
# reciprocals, divisions, square root
# ---------------------------------------------------------------------------------------------------------------------------
def _unequal_by_segment(I, idx):
    return {name: int(((idx >= s.start) & (idx < s.stop)).sum()) for name, s in I.seg.items() if ((idx >= s.start) & (idx < s.stop)).any()}


def test_rcp_nr():
    I = R.divisor_inputs(signed=True)
    d = I.x[0]
    got = dev("rcp_nr", d)[0]
    rep = R.div_report(got, np.ones_like(d), d)
    seg = _unequal_by_segment(I, rep["unequal"])
    record("rcp_nr", n=d.size, max_ulp=rep["max_ulp"], n_not_rn=rep["n_unequal"], not_rn_by_segment=seg,
           not_rn_inputs=[float(v).hex() for v in d[rep["unequal"]][:16]])
    assert rep["max_ulp"] <= 1.0, worst(I, np.bincount(rep["measured"], rep["err"], d.size))
    for name in ("random", "kernel"):
        assert name not in seg, f"rcp_nr is not RN(1/d) on {seg[name]} operands of the {name} set"


def test_rcp_pred():
    I = R.divisor_inputs(signed=False)
    d = I.x[0]
    assert np.all(d >= np.finfo(np.float64).tiny) and np.all(np.isfinite(d))
    got = dev("rcp_pred", d)[0]
    err = R.ulp_err_ld(got, LD(1) / d.astype(LD)).astype(np.float64)
    top = np.argsort(-err)[:200]                # the worst, exactly
    err[top] = R.frac_div_err(got[top], np.ones(top.size), d[top])
    record("rcp_pred", n=d.size, max_ulp=err.max())
    assert err.max() <= 11.0, worst(I, err)


@pytest.mark.parametrize("op", ["fdiv", "div_rcp"])
def test_quotients(op):
    I = R.quotient_inputs()
    a, b = I.x
    got = dev(op, a, b)[0]
    rep = R.div_report(got, a, b)
    seg = _unequal_by_segment(I, rep["unequal"])
    record(op, n=a.size, max_ulp=rep["max_ulp"], n_not_equal=rep["n_unequal"], not_equal_by_segment=seg,
           not_equal_inputs=[(float(a[i]).hex(), float(b[i]).hex()) for i in rep["unequal"][:16]])
    assert rep["max_ulp"] <= 1.0, worst(I, np.bincount(rep["measured"], rep["err"], a.size))
    for name in ("random", "kernel", "kernel_unit"):
        assert name not in seg, f"{op} differs from n / d on {seg[name]} operand pairs of the {name} set"


def test_sqrt_rsqrt():
    I = R.divisor_inputs(signed=False)
    x = I.x[0]
    sq, rsq = dev("sqrt_rsqrt", x)
    xl = x.astype(LD)
    err = R.ulp_err_ld(sq, np.sqrt(xl)).astype(np.float64)
    ne = np.flatnonzero(~R.bits_equal(sq, np.sqrt(x)))
    ref = LD(1) / np.sqrt(xl)
    rel = (np.abs(rsq.astype(LD) - ref) / ref).astype(np.float64)
    ns = I.seg["kernel"].start                  # structured (mantissa ends, powers of two) and the worst of the rest: mpmath
    st = np.unique(np.concatenate([np.arange(ns), np.argsort(-rel)[:500]]))
    mref = R.mp_rsqrt(x[st])
    rel[st] = R.mp_err(rsq[st], mref, unit=1.0) / np.array([float(v) for v in mref])
    record("sqrt_rsqrt", n=x.size, sq_max_ulp=err.max(), sq_n_not_rn=ne.size, sq_not_rn_by_segment=_unequal_by_segment(I, ne),
           rsq_max_rel=rel.max(), rsq_max_rel_in_2_53=rel.max() * 2.0 ** 53)
    assert err.max() <= 1.0, worst(I, err)
    # the final residual step fma(fma(-g, g, x), h, g) is there to round the root correctly (Markstein): on the kernels' own operands
    # and on the random set it has to (the mantissa ends and powers of two are held to 1 ulp, their count is recorded)
    seg = _unequal_by_segment(I, ne)
    for name in ("random", "kernel"):
        assert name not in seg, f"sqrt is not the correctly rounded root on {seg[name]} operands of the {name} set"
    assert rel.max() <= 2.0 ** -51, worst(I, rel)


# ---------------------------------------------------------------------------------------------------------------------------
# np_round5, wrap_pm_2pi
# ---------------------------------------------------------------------------------------------------------------------------
def test_np_round5_equals_numpy_bit_for_bit():
    """Measured on the MI355X: equal to np.round(x, 5) in value on all 1 400 005 inputs and in every bit on the 1 384 082 whose
    rounded value is not -0.  Where NumPy returns -0 (a negative input below 5e-6 in magnitude, -0 itself, the tie -5e-6) the
    device returns +0: div_rcp's residual fma(-b, q, a) is +0 + -0.  The one consumer takes fabs() of the result."""
    I = R.round5_inputs()
    x = I.x[0]
    got = np.concatenate([dev("np_round5", x[k:k + 300_000])[0] for k in range(0, x.size, 300_000)])
    ref = np.round(x, 5)
    neg0 = (ref == 0) & np.signbit(ref)
    ne = np.flatnonzero(~R.bits_equal(got, ref))
    record("np_round5", n=x.size, n_not_equal=ne.size, not_equal_by_segment=_unequal_by_segment(I, ne), n_reference_is_minus_zero=int(neg0.sum()),
           n_not_equal_in_value=int((got != ref).sum()))
    bad = ne[~neg0[ne]]
    assert bad.size == 0, [(I.name_of(i), float(x[i]).hex(), got[i], ref[i]) for i in bad[:8]]
    assert np.all(got[neg0] == 0.0) and not np.signbit(got[neg0]).any()    # the exception, held as it is: +0 for NumPy's -0


def test_wrap_pm_2pi_equals_the_numpy_loop():
    I = R.wrap_inputs()
    a = I.x[0]
    got = dev("wrap_pm_2pi", a)[0]
    ref = R.np_wrap_pm_2pi(a)
    ne = np.flatnonzero(~R.bits_equal(got, ref))
    record("wrap_pm_2pi", n=a.size, n_not_equal=ne.size)
    assert ne.size == 0, [(I.name_of(i), a[i], got[i], ref[i]) for i in ne[:8]]
    assert np.all(np.abs(got) <= R.TWO_PI)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan, 1e300, 100.00000000000001, -101.0])
def test_wrap_pm_2pi_refuses_what_its_loop_cannot_take(bad):
    """the loop runs |a| / 2 pi rounds and never ends for +-inf or 1e300: refused before anything is launched"""
    with pytest.raises(ValueError, match="wrap_pm_2pi"):
        dev("wrap_pm_2pi", np.array([0.5, bad, 1.0]))


# ---------------------------------------------------------------------------------------------------------------------------
# OBB-sum hull, OBB overlap
# ---------------------------------------------------------------------------------------------------------------------------
def test_obb_hull():
    """Every output against the exact hull, in ulps of hl + hw + |c1 - c0| (centre, extents) and of 1 (axis); the
    bound is twice the worst error of oracle.fxo_obb_hull on the same inputs, at least 2 ulp: device and oracle are two double
    evaluations of one definition that round independently.  Measured on the MI355X: centre 67 (bound 768), axis 1.16 (2),
    extents 2.58 (265).  The bisector form alone missed it at near-opposite headings -- 4.5e5 / 5.1e5 ulp (5e-10 m) at
    pi - 1e-6, 680 ulp at pi - 1e-13 -- which is why obb_hull forms the boxes' ranges one by one below |u0 + u1| = 0.0625."""
    I = R.hull_inputs()
    in0, in1, in2 = I.x
    got = np.stack(dev("obb_hull", in0, in1, in2), axis=1)
    scale = R.hull_scale(in0, in1, in2)
    ref = R.ld_hull(in0, in1, in2)
    e_dev, e_orc = R.hull_err_ld(got, ref, scale), R.hull_err_ld(R.oracle_hull(in0, in1, in2), ref, scale)
    ns = I.seg["random"].start                  # structured: mpmath
    mref = R.mp_hull(in0[:ns], in1[:ns], in2[:ns])
    e_dev[:ns] = R.hull_err_mp(got[:ns], mref, scale[:ns])
    e_orc[:ns] = R.hull_err_mp(R.oracle_hull(in0[:ns], in1[:ns], in2[:ns]), mref, scale[:ns])
    groups = {"centre": (0, 1), "axis": (2, 3), "extents": (4, 5)}
    fig = {}
    for name, cols in groups.items():
        o, d = e_orc[:, list(cols)].max(), e_dev[:, list(cols)].max()
        fig[name] = dict(oracle_max=float(o), bound=float(max(2.0, 2.0 * o)), device_max=float(d))
    record("obb_hull", n=in0.shape[0], **fig)
    for name, cols in groups.items():
        assert fig[name]["device_max"] <= fig[name]["bound"], (name, fig[name], worst(I, e_dev[:, list(cols)].max(1), cols=[in0, in1, in2]))
    # opposite and near-opposite headings (|u0 + u1| < 1e-12): the first box's axis, as the definition says
    for name in ("pi-1e-13", "opposite"):
        s = I.seg[name]
        assert np.all(np.hypot(in0[s, 2] + in1[s, 2], in0[s, 3] + in1[s, 3]) < 1e-12)
        assert np.array_equal(got[s, 2:4], in0[s, 2:4]), name


def test_obb_overlap():
    I = R.overlap_inputs()
    A, B = I.x
    got = dev("obb_overlap", A, B)[0]
    assert np.all((got == 0.0) | (got == 1.0))
    got = got == 1.0
    dec, tight = R.overlap_reference(A, B)
    robust = tight > 1e-9
    rnd = I.seg["random"]
    wrong = np.flatnonzero(robust & (got != dec))
    record("obb_overlap", n=A.shape[0], n_robust=int(robust.sum()), n_wrong_robust=wrong.size, random_inside_margin=int((~robust[rnd]).sum()),
           n_differ_inside_margin=int((~robust & (got != dec)).sum()))
    assert (~robust[rnd]).mean() <= 0.01
    assert wrong.size == 0, [(I.name_of(i), A[i].tolist(), B[i].tolist(), bool(got[i]), tight[i]) for i in wrong[:4]]
    for name in ("touch_edge", "touch_corner", "inside", "inside_rotated", "rotated_in_2^-20"):
        s = I.seg[name]
        assert dec[s].all() and got[s].all(), (name, int((~got[s]).sum()))
    for name in ("apart_2^-20", "rotated_apart_2^-20"):
        s = I.seg[name]
        assert not dec[s].any() and not got[s].any(), (name, int(got[s].sum()))


def test_selftest_refuses_bad_calls():
    with pytest.raises(ValueError, match="unknown op"):
        from frenetix_motion_planner_amd import _lib
        import ctypes as C
        pd = C.POINTER(C.c_double)
        _lib.check(_lib.lib().fx_device_selftest(99, 1, (pd * 4)(), (pd * 6)()))
    with pytest.raises(ValueError):
        dev("atan", np.zeros(0))
    with pytest.raises(ValueError):
        dev("atan", np.zeros((1 << 22) + 1))


# ---------------------------------------------------------------------------------------------------------------------------
def test_zz_measured_table():
    """(keep last) the figures of this run, printed; FXPLAN_RECORD_MEASURED=<file> writes them into that JSON file
    (profiles/device_math/measured.json was recorded that way)"""
    ops = ("atan", "atan_tab", "atan_small", "atan_small_tab", "sincos", "sincos_tab", "rcp_nr", "rcp_pred", "fdiv", "div_rcp",
           "sqrt_rsqrt", "np_round5", "wrap_pm_2pi", "obb_hull", "obb_overlap")
    missing = [op for op in ops if op not in MEASURED]
    if missing:
        pytest.skip(f"{missing} did not run in this process: nothing to sum")
    print("\n" + json.dumps(MEASURED, indent=1))
    path = os.environ.get("FXPLAN_RECORD_MEASURED")
    if path:
        old = json.load(open(path)) if os.path.exists(path) else {}
        old["device"] = MEASURED
        old["device_kernels_of_commit"] = os.environ.get("FXPLAN_MEASURED_COMMIT", old.get("device_kernels_of_commit", "unknown"))
        json.dump(old, open(path, "w"), indent=1, sort_keys=True)
