"""Exact references and input sets of the device arithmetic primitives (no GPU needed).

tests/test_device_math.py (`-m gpu`) holds every primitive of csrc/fx_math.h, fx_walk.h and fx_eval_kernel.h to these;
tests/test_device_math_ref.py holds the references to independent ones and the input sets to their coverage conditions.

References:
  division, reciprocal   fractions.Fraction on the exact binary values; the bulk through IEEE `/` (held to Fraction on samples)
  sqrt                   np.sqrt (correctly rounded); 1/sqrt in mpmath (200 bits), np.longdouble on the bulk
  atan, sin, cos         mpmath (200 bits) on the structured points, np.longdouble (64-bit significand: 2^-11 double-ulp) on the
                         bulk -- held to mpmath at 2^-9 double-ulp on samples, zeros of sin and cos included
  np_round5              np.round(x, 5), the operation the planner itself performs; wrap_pm_2pi: the same loop in NumPy double
  obb_hull               DESIGN 4.2 written out: mpmath on the structured points, the same text in np.longdouble on the bulk
  obb_overlap            the four-axis test in Fraction (exact: the margins of all four axes)
Structured points come first in every input set, so that a failure message names them.
"""
from fractions import Fraction

import mpmath   # (installed with torch's sympy; a missing mpmath is an error, not a skip)
import numpy as np

LD = np.longdouble
MP_PREC = 200
ATAN_EDGES = (0.4375, 0.6875, 1.1875, 2.4375)
TWO_PI = 6.283185307179586   # FX_TWO_PI
WRAP_MAX = 100.0             # FX_SELFTEST_WRAP_MAX: beyond it fx_device_selftest refuses wrap_pm_2pi input
CAR = (2.254, 0.805)         # half extents [m] (vehicle 2: 4.508 x 1.610)
TRUCK = (6.0, 1.275)


class Inputs:
    """An input set: named segments in order, concatenated.  x[k] = k-th operand, seg[name] = slice."""

    def __init__(self):
        self.parts, self.seg, self.n = [], {}, 0

    def add(self, name, *cols):
        cols = [np.atleast_1d(np.asarray(c, dtype=np.float64)) for c in cols]
        m = cols[0].shape[0]
        assert all(c.shape[0] == m for c in cols)
        self.seg[name] = slice(self.n, self.n + m)
        self.n += m
        self.parts.append(cols)
        return self

    @property
    def x(self):
        return [np.concatenate([p[k] for p in self.parts]) for k in range(len(self.parts[0]))]

    def name_of(self, i):
        for name, s in self.seg.items():
            if s.start <= i < s.stop:
                return f"{name}[{i - s.start}]"
        return str(i)


def _neighbours(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


# ---------------------------------------------------------------------------------------------------------------------------
# input sets
# ---------------------------------------------------------------------------------------------------------------------------
def atan_inputs():
    rng = np.random.default_rng(1401)
    e = np.array(ATAN_EDGES)
    I = Inputs()
    I.add("edges", _neighbours(np.concatenate([e, -e])))
    I.add("special", [0.0, -0.0, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 1e-300, -1e-300, 2.0 ** -27, -2.0 ** -27, 1e300, -1e300,
                      np.inf, -np.inf, np.nan])
    I.add("uniform64", rng.uniform(-64, 64, 100_000))
    I.add("loguniform", 10.0 ** rng.uniform(-300, 300, 100_000) * rng.choice([-1.0, 1.0], 100_000))
    I.add("small", rng.uniform(-0.4375, 0.4375, 50_000))
    # the three sets above leave [0.4375, 0.6875) with ~400 points: this one brings every interval of the reduction above 5 000
    I.add("reduction", rng.uniform(-2.4375, 2.4375, 49_000))
    return I


def atan_interval(x):
    """0 .. 4: which of the five intervals of the argument reduction |x| falls in (NaN: -1)."""
    ax = np.abs(x)
    return np.where(np.isnan(ax), -1, np.searchsorted(np.array(ATAN_EDGES), ax, side="right"))


def sincos_inputs():
    rng = np.random.default_rng(1402)
    k = np.arange(-200, 201)
    I = Inputs()
    I.add("k_pi_2", _neighbours(k * (np.pi / 2)))   # (k * fl(pi/2) in double: fl(k pi/2) up to an ulp; its neighbours are listed anyway)
    I.add("zero", [0.0, -0.0])
    I.add("uniform64", rng.uniform(-64, 64, 100_000))
    I.add("uniform1e6", rng.uniform(-1e6, 1e6, 100_000))
    return I


def sincos_quadrant(x):
    """(n & 3, n < 0) of the reduction n = rint(x * 2/pi), as fx_math.h forms it."""
    n = np.rint(x * 6.36619772367581382433e-01)
    return n.astype(np.int64) & 3, n < 0


def kernel_operands():
    """Divisors the kernels really form: T^2 .. T^5 as lon_coeffs builds them (and the quartic's 3 T^2, 4 T^2 T), segment lengths
    of the reference path, 1 + d'^2."""
    rng = np.random.default_rng(1403)
    T = np.arange(1, 101) * 0.1
    T2 = T * T
    T3 = T2 * T
    T4 = T3 * T
    T5 = T4 * T
    dp = rng.uniform(-10, 10, 20_000)
    return np.concatenate([T, T2, T3, T4, T5, 3.0 * T2, 4.0 * T2 * T, np.linspace(0.1, 1.0, 901), rng.uniform(0.1, 1.0, 2_000),
                           dp * dp + 1.0])


def _random_mantissas(rng, n, signed):
    v = np.ldexp(1.0 + rng.random(n), rng.integers(-40, 40, n))   # tools/micro/rcpacc.hip: (1 + u) * 2^e, e = -40 .. 39
    return v * rng.choice([-1.0, 1.0], n) if signed else v


def _mantissa_ends():
    below2 = np.float64(2.0) - np.arange(1, 2001) * np.spacing(1.0)        # all-ones mantissas first
    above1 = np.float64(1.0) + np.arange(0, 2000) * np.spacing(1.0)        # all-zeros first
    return below2, above1


def divisor_inputs(signed):
    """One-operand set of rcp_nr (signed) / rcp_pred and sqrt_rsqrt (positive normal numbers only: their callers guard the rest)."""
    rng = np.random.default_rng(1404)
    below2, above1 = _mantissa_ends()
    I = Inputs()
    I.add("below2", below2).add("above1", above1)
    I.add("pow2", np.ldexp(1.0, np.arange(-500, 501)))
    I.add("kernel", kernel_operands())
    I.add("random", _random_mantissas(rng, 200_000, signed))
    if signed:
        I.add("negative", -np.concatenate([below2[:200], above1[:200], kernel_operands()[:1000]]))
    return I


def quotient_inputs():
    """(numerator, divisor) set of fdiv and div_rcp."""
    rng = np.random.default_rng(1405)
    below2, above1 = _mantissa_ends()
    ko = kernel_operands()
    p2 = np.ldexp(1.0, np.arange(-300, 301))
    I = Inputs()
    I.add("below2", _random_mantissas(rng, below2.size, True), below2)
    I.add("above1", _random_mantissas(rng, above1.size, True), above1)
    I.add("ends_by_ends", np.concatenate([below2[:1000], above1[:1000]]), np.concatenate([above1[:1000], below2[:1000]]))
    I.add("pow2", _random_mantissas(rng, p2.size, True), p2)
    I.add("kernel", rng.uniform(-50, 50, ko.size), ko)
    I.add("kernel_unit", rng.uniform(-1, 1, ko.size), ko)          # (s - knot) / segment, normal / |normal|
    I.add("random", _random_mantissas(rng, 200_000, True), _random_mantissas(rng, 200_000, True))
    I.add("zero_numerator", np.array([0.0, -0.0, 0.0, -0.0]), np.array([3.0, 3.0, -0.7, -0.7]))
    return I


def round5_inputs():
    rng = np.random.default_rng(1406)
    k = np.arange(-200_000, 200_001)
    I = Inputs()
    I.add("zero", [0.0, -0.0])
    I.add("ties", _neighbours(k * 1e-5 + 5e-6))     # every decimal tie of the real range, and both neighbours
    I.add("yaw", rng.uniform(-10, 10, 100_000))
    I.add("loguniform", 10.0 ** rng.uniform(-12, 9, 100_000) * rng.choice([-1.0, 1.0], 100_000))
    return I


def wrap_inputs():
    rng = np.random.default_rng(1407)
    k = np.arange(-40, 41)
    I = Inputs()
    I.add("two_pi", _neighbours([TWO_PI, -TWO_PI]))
    I.add("zero", [0.0, -0.0])
    I.add("k_pi_2", k * (np.pi / 2))
    I.add("uniform64", rng.uniform(-64, 64, 100_000))
    assert np.all(np.abs(I.x[0]) <= WRAP_MAX)
    return I


HULL_DELTAS = (("equal", 0.0), ("1e-9", 1e-9), ("0.1", 0.1), ("pi/2", np.pi / 2), ("pi-1e-6", np.pi - 1e-6), ("pi-1e-13", np.pi - 1e-13),
               ("opposite", None))


def hull_inputs():
    """(c0x, c0y, u0x, u0y), (c1x, c1y, u1x, u1y), (hl, hw): headings as the kernels get them -- cos / sin in double."""
    rng = np.random.default_rng(1408)
    I = Inputs()
    for name, delta in HULL_DELTAS:
        rows = []
        for hl, hw in (CAR, TRUCK):
            for sep in (0.0, 0.1, 1.0, 5.0):
                for _ in range(8):
                    th0, phi = rng.uniform(-np.pi, np.pi, 2)
                    c0 = rng.uniform(-295, 295, 2)
                    c1 = c0 + sep * np.array([np.cos(phi), np.sin(phi)])
                    u0 = np.array([np.cos(th0), np.sin(th0)])
                    u1 = -u0 if delta is None else np.array([np.cos(th0 + delta), np.sin(th0 + delta)])
                    rows.append(np.concatenate([c0, u0, c1, u1, [hl, hw]]))
        r = np.array(rows)
        I.add(name, r[:, 0:4], r[:, 4:8], r[:, 8:10])
    n = 20_000
    th0, phi = rng.uniform(-np.pi, np.pi, (2, n))
    # consecutive steps turn by a little; a fifth of the pairs by anything
    delta = np.where(rng.random(n) < 0.8, rng.normal(size=n) * 0.1, rng.uniform(-np.pi, np.pi, n))
    sep = rng.uniform(0, 5, n)
    c0 = rng.uniform(-295, 295, (n, 2))
    c1 = c0 + sep[:, None] * np.stack([np.cos(phi), np.sin(phi)], axis=1)
    ext = np.where((rng.random(n) < 0.5)[:, None], np.array(CAR), np.array(TRUCK))
    I.add("random", np.column_stack([c0, np.cos(th0), np.sin(th0)]), np.column_stack([c1, np.cos(th0 + delta), np.sin(th0 + delta)]), ext)
    return I


def overlap_inputs():
    """Two stored boxes (cx, cy, ex, ey, h1, h2) each."""
    rng = np.random.default_rng(1409)
    I = Inputs()

    def box(c, th, h):
        c, th, h = np.atleast_2d(c), np.atleast_1d(th), np.atleast_2d(h)
        return np.column_stack([c, np.cos(th), np.sin(th), h])

    # axis-aligned, integer coordinates (axes (1, 0) / (0, 1) / (-1, 0) exactly): every operation of the test is exact
    axes = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    edge, corner, inside, apart = [], [], [], []
    for ea in axes:
        for eb in axes:
            for (h1, h2, g1, g2) in ((2, 1, 3, 1), (1, 1, 1, 1), (5, 2, 1, 4), (3, 3, 2, 7)):
                # extents of both boxes along world x / y
                ax_, ay_ = (h1, h2) if ea[1] == 0 else (h2, h1)
                bx_, by_ = (g1, g2) if eb[1] == 0 else (g2, g1)
                for cx, cy in ((10, -7), (-120, 33), (0, 0)):
                    A = [cx, cy, ea[0], ea[1], h1, h2]
                    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1)):   # touching along an edge
                        off = (sx * (ax_ + bx_), sy * (ay_ + by_))
                        edge.append(A + [cx + off[0], cy + off[1], eb[0], eb[1], g1, g2])
                        gap = 2.0 ** -20
                        apart.append(A + [cx + off[0] + sx * gap, cy + off[1] + sy * gap, eb[0], eb[1], g1, g2])
                    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):  # touching at a corner
                        corner.append(A + [cx + sx * (ax_ + bx_), cy + sy * (ay_ + by_), eb[0], eb[1], g1, g2])
                    inside.append([cx, cy, ea[0], ea[1], 10 * h1, 10 * h2, cx + 1, cy - 1, eb[0], eb[1], 0.25, 0.5])
    for name, rows in (("touch_edge", edge), ("touch_corner", corner), ("apart_2^-20", apart), ("inside", inside)):
        r = np.array(rows, dtype=np.float64)
        I.add(name, r[:, :6], r[:, 6:])
    # rotated pairs 2^-20 apart along the first box's axis (the decision is exact in Fraction; the device's rounding is ~1e-15)
    m = 500
    th = rng.uniform(-np.pi, np.pi, m)
    ha, hb = rng.uniform(0.5, 6, (m, 2)), rng.uniform(0.5, 6, (m, 2))
    ca = rng.uniform(-295, 295, (m, 2))
    e = np.stack([np.cos(th), np.sin(th)], axis=1)
    for name, gap in (("rotated_apart_2^-20", 2.0 ** -20), ("rotated_in_2^-20", -(2.0 ** -20))):
        cb = ca + (ha[:, :1] + hb[:, :1] + gap) * e
        I.add(name, box(ca, th, ha), box(cb, th, hb))
    n = 20_000
    ca = rng.uniform(-295, 295, (n, 2))
    cb = ca + rng.normal(size=(n, 2)) * 5.0
    I.add("random", box(ca, rng.uniform(-np.pi, np.pi, n), np.where((rng.random(n) < 0.5)[:, None], np.array(CAR), np.array(TRUCK))),
          box(cb, rng.uniform(-np.pi, np.pi, n), rng.uniform(0.3, 8, (n, 2))))
    # contained: a small box well inside a large one, any orientation
    m = 1_000
    ca = rng.uniform(-295, 295, (m, 2))
    I.add("inside_rotated", box(ca, rng.uniform(-np.pi, np.pi, m), rng.uniform(5, 8, (m, 2))),
          box(ca + rng.uniform(-1, 1, (m, 2)), rng.uniform(-np.pi, np.pi, m), rng.uniform(0.1, 1, (m, 2))))
    return I


# ---------------------------------------------------------------------------------------------------------------------------
# error measures
# ---------------------------------------------------------------------------------------------------------------------------
def ulp_of(ref):
    """Spacing of doubles at the (correctly rounded) reference value."""
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float64)))


def ulp_err_ld(got, ref_ld):
    """|got - ref| in ulps of the reference, reference in np.longdouble."""
    ref_ld = np.asarray(ref_ld, dtype=LD)
    return np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref_ld) / ulp_of(ref_ld.astype(np.float64)).astype(LD)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.view(np.uint64) == b.view(np.uint64)


def _mp(x):
    return mpmath.mpf(float(x))


def mp_of_ld(v):
    """An np.longdouble as an mpf, exactly (two doubles)."""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(LD(v) - LD(hi)))


def mp_ulp_err(got, ref_mp):
    """|got - ref| in ulps of the reference for one value, reference an mpmath number (NaN / inf handled by the callers)."""
    with mpmath.workprec(MP_PREC):
        r = float(ref_mp)
        return float(abs(_mp(got) - ref_mp) / _mp(np.spacing(abs(r)) if r != 0 else 5e-324))


def mp_unary(fn, x):
    """fn in mpmath at MP_PREC bits on every (finite) x: list of mpf."""
    with mpmath.workprec(MP_PREC):
        return [fn(_mp(v)) for v in x]


def mp_atan(x): return mp_unary(mpmath.atan, x)
def mp_sin(x): return mp_unary(mpmath.sin, x)
def mp_cos(x): return mp_unary(mpmath.cos, x)
def mp_rsqrt(x): return mp_unary(lambda v: 1 / mpmath.sqrt(v), x)


def mp_err(got, ref_mp_list, unit=None):
    """Errors of `got` against a list of mpf: in ulps of each reference (unit None) or in units of `unit` (absolute)."""
    out = np.empty(len(ref_mp_list))
    with mpmath.workprec(MP_PREC):
        for i, (g, r) in enumerate(zip(got, ref_mp_list)):
            d = abs(_mp(g) - r)
            out[i] = float(d / _mp(unit)) if unit is not None else float(d / _mp(np.spacing(abs(float(r))) if float(r) != 0 else 5e-324))
    return out


# ---- Fraction: division --------------------------------------------------------------------------------------------------
def frac_div(a, b):
    """(RN(a / b) as float, exact quotient) of two finite doubles, b != 0."""
    q = Fraction(float(a)) / Fraction(float(b))
    return float(q), q   # Fraction.__float__ is integer true division: correctly rounded


def frac_div_err(got, a, b):
    """Exact error of `got` against a / b in ulps of RN(a / b), for arrays (slow: ~10 us per element)."""
    out = np.empty(len(got))
    for i, (g, x, y) in enumerate(zip(got, a, b)):
        rn, q = frac_div(x, y)
        u = Fraction(float(np.spacing(abs(rn)))) if rn != 0 else Fraction(5e-324)
        out[i] = float(abs(Fraction(float(g)) - q) / u)
    return out


def div_report(got, a, b, sample=2_000, seed=7):
    """Error of a device quotient in ulps of the correctly rounded a / b.  Elements bit-equal to IEEE `a / b` are within half an
    ulp by definition (`/` itself is held to Fraction on a sample here and in the CPU module); every other element, and a seeded
    sample of all, is measured exactly in Fraction.  Returns dict(max_ulp, n_unequal, unequal (indices), err (per measured index))."""
    got, a, b = (np.asarray(v, dtype=np.float64) for v in (got, a, b))
    with np.errstate(all="ignore"):
        rn = a / b
    eq = bits_equal(got, rn)
    idx = np.flatnonzero(~eq)
    rng = np.random.default_rng(seed)
    smp = rng.choice(got.size, min(sample, got.size), replace=False)
    # IEEE division against Fraction on the sample (a wrong `/` would make "bit-equal" meaningless)
    for i in smp[:500]:
        assert frac_div(a[i], b[i])[0] == rn[i] or (rn[i] == 0 and frac_div(a[i], b[i])[0] == 0), (a[i], b[i])
    measured = np.unique(np.concatenate([idx, smp]))
    err = frac_div_err(got[measured], a[measured], b[measured]) if measured.size else np.zeros(0)
    return dict(max_ulp=float(err.max()) if err.size else 0.0, n_unequal=int(idx.size), unequal=idx, measured=measured, err=err)


def np_wrap_pm_2pi(a):
    """wrap_pm_2pi's loop in NumPy double, elementwise."""
    a = np.array(a, dtype=np.float64)
    assert np.all(np.abs(a) <= WRAP_MAX)
    while True:
        m = a > TWO_PI
        if not m.any():
            break
        a[m] = a[m] - TWO_PI
    while True:
        m = a < -TWO_PI
        if not m.any():
            break
        a[m] = a[m] + TWO_PI
    return a


# ---- OBB-sum hull, DESIGN 4.2 --------------------------------------------------------------------------------------------
def _hull_generic(c0, u0, c1, u1, hl, hw, sqrt, absf, lt, mn_, mx_):
    """axis e1 = normalize(u0 + u1), or u0 where |u0 + u1| < 1e-12; e2 = perp(e1); extents = the tight range of both boxes' eight
    corners on (e1, e2); centre = the middle of that range.  Scalar arithmetic of whatever number type comes in."""
    mx, my = u0[0] + u1[0], u0[1] + u1[1]
    n = sqrt(mx * mx + my * my)
    if lt(n):
        ex, ey = u0[0], u0[1]
    else:
        ex, ey = mx / n, my / n
    fx, fy = -ey, ex
    p1, p2 = [], []
    for c, u in ((c0, u0), (c1, u1)):
        vx, vy = -u[1], u[0]
        for a in (1, -1):
            for b in (1, -1):
                qx, qy = c[0] + a * hl * u[0] + b * hw * vx, c[1] + a * hl * u[1] + b * hw * vy
                p1.append(qx * ex + qy * ey)
                p2.append(qx * fx + qy * fy)
    lo1, hi1, lo2, hi2 = mn_(p1), mx_(p1), mn_(p2), mx_(p2)
    m1, m2 = (lo1 + hi1) / 2, (lo2 + hi2) / 2
    return (m1 * ex + m2 * fx, m1 * ey + m2 * fy, ex, ey, (hi1 - lo1) / 2, (hi2 - lo2) / 2)


def mp_hull(in0, in1, in2):
    """The hull of every row in mpmath: list of 6-tuples of mpf."""
    out = []
    with mpmath.workprec(MP_PREC):
        thr = mpmath.mpf(1e-12)
        for p, q, h in zip(in0, in1, in2):
            P, Q, H = [_mp(v) for v in p], [_mp(v) for v in q], [_mp(v) for v in h]
            out.append(_hull_generic(P[0:2], P[2:4], Q[0:2], Q[2:4], H[0], H[1], mpmath.sqrt, abs, lambda n: n < thr, min, max))
    return out


def ld_hull(in0, in1, in2):
    """The same definition in np.longdouble, vectorised over the rows: [n][6]."""
    P, Q, H = (np.asarray(v, dtype=np.float64).astype(LD) for v in (in0, in1, in2))
    mx, my = P[:, 2] + Q[:, 2], P[:, 3] + Q[:, 3]
    n = np.sqrt(mx * mx + my * my)
    flat = n < LD(1e-12)
    nn = np.where(flat, LD(1), n)
    ex, ey = np.where(flat, P[:, 2], mx / nn), np.where(flat, P[:, 3], my / nn)
    fx, fy = -ey, ex
    p1, p2 = [], []
    for B in (P, Q):
        ux, uy = B[:, 2], B[:, 3]
        vx, vy = -uy, ux
        for a in (1, -1):
            for b in (1, -1):
                qx, qy = B[:, 0] + a * H[:, 0] * ux + b * H[:, 1] * vx, B[:, 1] + a * H[:, 0] * uy + b * H[:, 1] * vy
                p1.append(qx * ex + qy * ey)
                p2.append(qx * fx + qy * fy)
    p1, p2 = np.stack(p1), np.stack(p2)
    lo1, hi1, lo2, hi2 = p1.min(0), p1.max(0), p2.min(0), p2.max(0)
    m1, m2 = (lo1 + hi1) / 2, (lo2 + hi2) / 2
    return np.stack([m1 * ex + m2 * fx, m1 * ey + m2 * fy, ex, ey, (hi1 - lo1) / 2, (hi2 - lo2) / 2], axis=1)


def hull_scale(in0, in1, in2):
    """The unit of the centre's and the extents' error: ulp of hl + hw + |c1 - c0|."""
    in0, in1, in2 = (np.asarray(v, dtype=np.float64) for v in (in0, in1, in2))
    return np.spacing(in2[:, 0] + in2[:, 1] + np.hypot(in1[:, 0] - in0[:, 0], in1[:, 1] - in0[:, 1]))


def hull_err_ld(got6, ref_ld, scale):
    """[n][6] errors: centre and extents in ulps of (hl + hw + |c1 - c0|), axis in ulps of 1."""
    d = np.abs(np.asarray(got6, dtype=np.float64).astype(LD) - ref_ld)
    unit = np.stack([scale, scale, np.full_like(scale, np.spacing(1.0)), np.full_like(scale, np.spacing(1.0)), scale, scale], axis=1)
    return (d / unit.astype(LD)).astype(np.float64)


def hull_err_mp(got6, ref_mp, scale):
    out = np.empty((len(ref_mp), 6))
    with mpmath.workprec(MP_PREC):
        one = _mp(np.spacing(1.0))
        for i, (g, r) in enumerate(zip(got6, ref_mp)):
            s = _mp(scale[i])
            for k in range(6):
                out[i, k] = float(abs(_mp(g[k]) - r[k]) / (one if k in (2, 3) else s))
    return out


def oracle_hull(in0, in1, in2):
    """oracle.fxo_obb_hull on every row: [n][6]."""
    import ctypes as C
    from oracle import oracle
    L = oracle.lib()
    pd = C.POINTER(C.c_double)
    in0, in1, in2 = (np.ascontiguousarray(v, dtype=np.float64) for v in (in0, in1, in2))
    out = np.zeros((in0.shape[0], 6))
    p0, p1, po = in0.ctypes.data, in1.ctypes.data, out.ctypes.data   # rows by address: 4, 4 and 6 doubles
    hl, hw = in2[:, 0].tolist(), in2[:, 1].tolist()
    f, cast = L.fxo_obb_hull, C.cast
    for i in range(in0.shape[0]):
        f(cast(p0 + 32 * i, pd), cast(p0 + 32 * i + 16, pd), cast(p1 + 32 * i, pd), cast(p1 + 32 * i + 16, pd), hl[i], hw[i],
          cast(po + 48 * i, pd))
    return out


# ---- OBB overlap: four-axis SAT, exact -----------------------------------------------------------------------------------
def frac_overlap(a, b):
    """(overlap, margins): margins[k] = |t . axis_k| - (sum of the radii on axis k), exact; separated <=> some margin > 0
    (strict, touching collides)."""
    a, b = [Fraction(float(v)) for v in a], [Fraction(float(v)) for v in b]
    tx, ty = b[0] - a[0], b[1] - a[1]
    c = a[2] * b[2] + a[3] * b[3]
    s = a[2] * b[3] - a[3] * b[2]
    ac, as_ = abs(c), abs(s)
    g = (abs(tx * a[2] + ty * a[3]) - (a[4] + (b[4] * ac + b[5] * as_)),
         abs(-tx * a[3] + ty * a[2]) - (a[5] + (b[4] * as_ + b[5] * ac)),
         abs(tx * b[2] + ty * b[3]) - (b[4] + (a[4] * ac + a[5] * as_)),
         abs(-tx * b[3] + ty * b[2]) - (b[5] + (a[4] * as_ + a[5] * ac)))
    return not any(v > 0 for v in g), g


def ld_overlap_margin(A, B):
    """max over the four axes of the margin, in np.longdouble, vectorised: > 0 <=> separated."""
    a, b = np.asarray(A, dtype=np.float64).astype(LD), np.asarray(B, dtype=np.float64).astype(LD)
    tx, ty = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
    c = a[:, 2] * b[:, 2] + a[:, 3] * b[:, 3]
    s = a[:, 2] * b[:, 3] - a[:, 3] * b[:, 2]
    ac, as_ = np.abs(c), np.abs(s)
    g = np.stack([np.abs(tx * a[:, 2] + ty * a[:, 3]) - (a[:, 4] + (b[:, 4] * ac + b[:, 5] * as_)),
                  np.abs(-tx * a[:, 3] + ty * a[:, 2]) - (a[:, 5] + (b[:, 4] * as_ + b[:, 5] * ac)),
                  np.abs(tx * b[:, 2] + ty * b[:, 3]) - (b[:, 4] + (a[:, 4] * ac + a[:, 5] * as_)),
                  np.abs(-tx * b[:, 3] + ty * b[:, 2]) - (b[:, 5] + (a[:, 4] * as_ + a[:, 5] * ac))])
    return g.max(0)


LD_DECIDES = 1e-3   # a margin this far from 0 is decided by the longdouble form (its rounding: ~1e-16 of a few hundred metres)


def overlap_reference(A, B, exact_all=False):
    """Exact decisions [n] (bool) and the distance of each decision from flipping [n] -- |largest of the four margins|: a separated
    pair overlaps once it falls to 0, an overlapping pair separates once it rises above 0.  Fraction wherever the margin is
    within LD_DECIDES of 0 (or everywhere: exact_all); farther out the longdouble form decides, held to Fraction by the CPU module."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    gm = ld_overlap_margin(A, B)
    dec, tight = ~(gm > 0), np.abs(gm).astype(np.float64)
    for i in (range(len(A)) if exact_all else np.flatnonzero(tight < LD_DECIDES)):
        d, g = frac_overlap(A[i], B[i])
        dec[i], tight[i] = d, float(abs(max(g)))
    return dec, tight
