"""High-precision values and derived rounding bounds for the interceptor: right-hand side, control and Hamiltonian in both charts and
both stages, the chart change, and short trajectories (helper of test_interceptor_pin_cpu.py, test_gpu_interceptor_pin.py and
golden/make_interceptor_pin_golden.py, not a test).  The kits, the error model and the decidability rule are those of
fast_reference.py; this module restates the model once over the kit interface:

  interceptor_ref   common, control_k, rhs_ref, hamiltonian, jac_chart1, jac_chart2, lu6_solve, change_chart, set_chart, rk4_step,
                    compute_traj in the reference's operation order, as oracle/interceptor_oracle.c and InterceptorT<false>
                    (socp_amd/csrc/models_interceptor.hpp) write them;
  interceptor_fast  rhs_fast as InterceptorT<true> writes it: reciprocals instead of divisions, tan = sin / cos, cos(beta) and
                    sin(beta) from the atan2 arguments bx, by through rsqrt (with the b2 > 0 test and the rescaling of (bx, by) where
                    b2 is not comfortably normal), copysign saturation, the short sincos.  Everything else is shared.

Budgets.  rcp, rsqrt: C_RCP = C_RSQ = 2.  exp_glibc (common() of both flavours): C_EXP = 2; the library exp of rhs_fast: C_EXP_LIB = 6.
The library's sin / cos 8u, tan 10u, atan2 12u, acos 8u (fast_reference.py says where these come from: a specification).

ifast::sincos (C_SINCOS_FAST, K_ABS_SINCOS_FAST), derived from its text for |x| <= 1e4, that is |k| <= 6367:
  reduction  k = rint(x 2/pi); r1 = fma(-k, P1, x) is EXACT: for k != 0, |x| > 1/2, so x and k P1 are multiples of 2^-53, and so is
             their difference, which is below 1 in magnitude (|r1| <= pi/4 (1 + 1e-12): the product x 2/pi is off by 2 ulp at most) and
             hence a double.  r = fma(-k, P2, r1) is one rounding, u|r|.  P1 + P2 misses pi/2 by |P3| < 2^-109 (1.4975e-33 < 1.5408e-33),
             so r misses x - k pi/2 by at most |k| 2^-109 + u|r|: ABSOLUTE in its first part, which is why the budget has two parts.
  sin        sr = fma(r r2, p, r), p the degree-6 Horner polynomial in r2 = r^2 with |p| <= 1/6.  Taylor remainder r^17/17! <= 4.6e-17
             <= 0.6u|sin r| at |r| = pi/4 (the ratio only falls below that).  Roundings: the last fma 1u; r r2 and r2 (u each) and p
             (its own last fma u, the earlier ones scaled by r2/20 and less: < 1.1u together) enter through r^3 p, at most
             (pi/4)^2/6 = 0.103 of the result: 3.1 * 0.103 < 0.33u.  The reduction's u|r| times |r cos r / sin r| <= 1.
             Sum 1 + 0.33 + 1 + 0.6 < 3u.
  cos        cr = fma(r2 r2, q, fma(-1/2, r2, 1)), cos r >= 0.7071.  Inner fma: u (its value 1 - r2/2 <= 1, so <= 1.42u of the result);
             r2's rounding through r2/2 <= 0.31: 0.44u; r2 r2 q <= 0.016 with ~3 roundings: 0.07u; last fma 1u; remainder r^18/18! =
             2e-18 < 0.03u; the reduction's u|r| times |r tan r| <= 0.79.  Sum < 3.8u.
  Doubled, as C_RCP and C_RSQ are:  C_SINCOS_FAST = 8 (relative, in u) and K_ABS_SINCOS_FAST = 2^-108 |k| |d/dx| (absolute).
  The quadrant selection is exact.  Rows with an angle beyond 1e4 in magnitude are not in the fixture.

Decisions recorded as margins (fast_reference.py: decidable when every margin exceeds 4x its error): the saturation |u| > u_max; in
rhs_fast b2 > 0 and the two range tests of b2; stage == 1 and a1 == +-pi/2 compare inputs (error zero); in the chart change the sign
tests c1 s2 < 0 (c1 c2 > 0), |sinPhi| < eps, s1/cn < 0 / > 0, sinPhi > 0, and every pivot choice (the margin is the chosen pivot's lead
over the runner-up; flipped, the runner-up is taken: the same linear system, another elimination order); |cos a1| >= chartLimit.

Signed zeros: mpf carries none.  atan2(+-0, x < 0) = +-pi is the one place the model reads the sign of a zero (beta with p_a2 = +-0.0):
the sign bit of the input travels beside the number (`by_negative_zero`)."""
import fractions

import numpy as np

import fast_reference as fr
from fast_reference import F64, C_EXP, C_EXP_LIB, F64Kit, MpfKit, TrackedKit, Tracked, mpf, mpmath, U

(C0, HR, D0, ETA, PROP, EMPTY, Q, VE, ALPHA_MAX, UMAX, AMAX, MU_GFT, MUT, MUV, MUC, REARTH, MU0, CHART_LIMIT) = range(18)
SHIPPED = np.array([0.00075, 7500, 0.00005, 0.442, 200, 200, 10, 1500, np.pi / 6, 1, 1500, 1, 0, 1, 0, 6378145, 3.986e14, 0.1])
PI = float(np.pi)
EPS = 1e-18
C_SINCOS_FAST = 8
SINCOS_FAST_RANGE = 1e4
B2_LO, B2_HI, B2_SCALE = 2.0 ** -900, 2.0 ** 900, 2.0 ** 600        # rhs_fast: (bx, by) rescaled where b2 is outside [lo, hi]
P1, P2 = float.fromhex("0x1.921fb54442d18p+0"), float.fromhex("0x1.1a62633145c07p-54")
TWO_OVER_PI = 0.6366197723675814
SIN_COEF = [-1.0 / 1307674368000.0, 1.0 / 6227020800.0, -1.0 / 39916800.0, 1.0 / 362880.0, -1.0 / 5040.0, 1.0 / 120.0, -1.0 / 6.0]
COS_COEF = [1.0 / 20922789888000.0, -1.0 / 87178291200.0, 1.0 / 479001600.0, -1.0 / 3628800.0, 1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0]


def fma64(a, b, c):
    """A correctly rounded fused multiply-add of three doubles."""
    return F64(float(fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c))))


def sincos_fast_f64(x, mutation=None):
    """ifast::sincos operation for operation in float64."""
    x = F64(x)
    k = np.rint(x * F64(TWO_OVER_PI))
    r = fma64(-k, P1, x)
    if mutation != "pio2_tail_dropped":
        r = fma64(-k, P2, r)
    r2 = r * r
    p = F64(SIN_COEF[0])
    for c in SIN_COEF[1:]:
        p = fma64(p, r2, c)
    sr = fma64(r * r2, p, r)
    q = F64(COS_COEF[0])
    for c in COS_COEF[1:]:
        q = fma64(q, r2, c)
    cr = fma64(r2 * r2, q, fma64(-0.5, r2, 1.0))
    n = int(k)
    s0, c0 = (cr, sr) if n & 1 else (sr, cr)
    return (-s0 if n & 2 else s0), (-c0 if (n + 1) & 2 else c0)


def _sincos_fast(K, a):
    """(sin a, cos a) as ifast::sincos forms them, on the kit's numbers."""
    if isinstance(K, F64Kit):
        return sincos_fast_f64(a, getattr(K, "mutation", None))
    if hasattr(K, "sincos_fast"):                                         # dopri5_reference.D5Tracked: the same budget on its numbers
        assert abs(a.v) <= SINCOS_FAST_RANGE + 1, "outside the range ifast::sincos' budget is derived for"
        return K.sincos_fast(a, C_SINCOS_FAST, abs(mpmath.nint(a.v * 2 / mpmath.pi)) * mpf(2) ** -108)
    if isinstance(K, TrackedKit):
        assert abs(a.v) <= SINCOS_FAST_RANGE + 1, "outside the range ifast::sincos' budget is derived for"
        s, c = mpmath.sin(a.v), mpmath.cos(a.v)
        k_abs = abs(mpmath.nint(a.v * 2 / mpmath.pi)) * mpf(2) ** -108
        return (Tracked(s, abs(c) * (a.e + k_abs) + C_SINCOS_FAST * U * abs(s)),
                Tracked(c, abs(s) * (a.e + k_abs) + C_SINCOS_FAST * U * abs(c)))
    return mpmath.sin(a), mpmath.cos(a)


def _mut(K):
    return getattr(K, "mutation", None)


# ---- the model, once -------------------------------------------------------------------------------------------------------

def common(K, P, stage, t, h, rcp=False, exp=None):
    """(mass, c_max, d, r, g, ft): the temporaries of Model_k / Control_k / Hamiltonian_k with ComputeMass.  stage is 0 or 1 (an input
    compared exactly).  rcp: as rhs_fast forms them."""
    exp = exp or K.exp
    qm1 = P[Q] * P[MU_GFT]
    powered = stage == 1
    if rcp:
        tm = t if powered or _mut(K) == "coast_mass_t" else P[PROP] * K.rcp(P[Q])
        mass = P[EMPTY] + P[PROP] - qm1 * tm
        im, ihr = K.rcp(mass), K.rcp(P[HR])
        dens = exp(-h * ihr) * (P[PROP] + P[EMPTY]) * im
        r = h + P[REARTH]
        ir = K.rcp(r)
        return dict(mass=mass, im=im, ihr=ihr, c_max=P[C0] * dens, d=P[D0] * dens, r=r, ir=ir, g=P[MU0] * ir * ir * P[MU_GFT],
                    ft=P[VE] * (stage * qm1))
    t1 = P[PROP] / P[Q]
    qm = stage * P[Q] * P[MU_GFT]
    mass = P[EMPTY] + P[PROP] - qm1 * (t if powered or _mut(K) == "coast_mass_t" else t1)
    e = exp(-h / P[HR])
    r = h + P[REARTH]
    return dict(mass=mass, c_max=P[C0] * e * (P[PROP] + P[EMPTY]) / mass, d=P[D0] * e * (P[PROP] + P[EMPTY]) / mass, r=r,
                g=P[MU0] / r / r * P[MU_GFT], ft=P[VE] * qm)


def control_k(K, P, c, chart1, v, c1, p_v, p_a1, p_a2, neg0):
    """Control_1 / Control_2: (u, beta, sb, cb).  neg0: the sign bit of the input p_a2."""
    mass, c_max, ft, alpha_max, eta = c["mass"], c["c_max"], c["ft"], P[ALPHA_MAX], P[ETA]
    beta = K.atan2(p_a2, p_a1 * c1, neg0) if chart1 else K.atan2(-p_a2, p_a1 * c1, not neg0)
    sb, cb = K.sin(beta), K.cos(beta)
    A = p_a1 * (v * c_max * cb + ft * cb * alpha_max / mass / v)
    B = p_a2 * (v * c_max * sb / c1 + ft * sb / c1 * alpha_max / mass / v)
    den = p_v * (2 * eta * c_max * v * v + ft * alpha_max * alpha_max / mass) - P[MUC]
    u = ((A + B) if chart1 else (A - B)) / den
    if K.cmp("|u|-u_max", abs(u) - P[UMAX], ">"):
        u = P[UMAX] * u / abs(u)
    return u, beta, sb, cb


def _terms(K, P, chart, stage, t, X, neg0):
    c = common(K, P, stage, t, X[0])
    s1, c1, s2, c2 = K.sin(X[2]), K.cos(X[2]), K.sin(X[3]), K.cos(X[3])
    u, beta, sb, cb = control_k(K, P, c, chart == 1, X[1], c1, X[7], X[8], X[9], neg0)
    alpha = P[ALPHA_MAX] * u
    return c, s1, c1, s2, c2, u, beta, sb, cb, K.sin(alpha), K.cos(alpha)


def rhs_ref(K, P, chart, stage, t, X, neg0=False):
    """Model_1 / Model_2 in the reference's order.  Returns (Xdot[12], [u, beta])."""
    c, s1, c1, s2, c2, u, beta, sb, cb, sa, ca = _terms(K, P, chart, stage, t, X, neg0)
    v, L = X[1], X[4]
    p_h, p_v, p_a1, p_a2, p_L, p_l = X[6:12]
    mass, c_max, d, r, g, ft, eta, hr = c["mass"], c["c_max"], c["d"], c["r"], c["g"], c["ft"], P[ETA], P[HR]
    sL, cL, tL = K.sin(L), K.cos(L), K.tan(L)
    o = [None] * 12
    if chart == 1:
        sg, cg, sc, cc, p_gamma, p_chi = s1, c1, s2, c2, p_a1, p_a2
        o[0] = v * sg
        o[1] = -(d + eta * c_max * u * u) * v * v - g * sg + ft * ca / mass
        o[2] = v * c_max * u * cb - g / v * cg + ft * sa * cb / mass / v + v * cg / r
        o[3] = v * c_max * u * sb / cg + ft * sa * sb / cg / mass / v + v * cg * tL * sc / r
        o[4] = v * cg * cc / r
        o[5] = v * cg * sc / cL / r
        o[6] = (-p_v / hr * (d + eta * c_max * u * u) * v * v - 2 * g / r * (p_gamma / v * cg + p_v * sg)
                + p_L * v * cg * cc / r / r + p_gamma * v * cg / r / r + p_gamma * v * c_max * u * cb / hr
                + p_l * v * cg * sc / cL / r / r + p_chi * v * cg * tL * sc / r / r + p_chi * v * c_max * u * sb / cg / hr)
        o[7] = -(p_L * cg * cc / r + p_l * cg * sc / cL / r + p_h * sg
                 + p_gamma * (c_max * u * cb + g / v / v * cg - ft * sa * cb / mass / v / v + cg / r)
                 + p_chi * (c_max * u * sb / cg - ft * sa * sb / cg / mass / v / v + cg * tL * sc / r)
                 - p_v * 2 * (d + eta * c_max * u * u) * v)
        o[8] = (v * (p_L * sg * cc / r + p_l * sg * sc / cL / r - p_h * cg)
                - g * (p_gamma / v * sg - p_v * cg)
                + p_gamma * v * sg / r + p_chi * v * sg * tL * sc / r
                - p_chi * (v * c_max * u * sb + ft * sa * sb / mass / v) * sg / cg / cg)
        o[9] = v * (p_L * cg * sc / r - p_l * cg * cc / cL / r - p_chi * cg * tL * cc / r)
        o[10] = -p_l * v * cg * sc * sL / cL / cL / r - p_chi * v * cg * (1 + tL * tL) * sc / r
    else:
        st, ct, sp, cp, p_theta, p_phi = s1, c1, s2, c2, p_a1, p_a2
        tt = K.tan(X[2])
        o[0] = -v * ct * cp
        o[1] = -(d + eta * c_max * u * u) * v * v + g * ct * cp + ft * ca / mass
        o[2] = v * c_max * u * cb + v * st * (cp + sp * tL) / r + (ft * sa * cb / (mass * v) - g * st * cp / v)
        o[3] = (-v * c_max * u * sb / ct + v * ct * (sp + tt * tt * (sp - tL * cp)) / r
                - (ft * sa * sb / (mass * v * ct) + g * sp / (v * ct)))
        o[4] = v * ct * sp / r
        o[5] = v * st / (r * cL)
        o[6] = (-p_v / hr * (d + eta * c_max * u * u) * v * v - 2 * g / r * (p_theta * st * cp / v + p_phi * sp / ct / v - p_v * ct * cp)
                + p_L * v * ct * sp / r / r + v * p_theta * st * (cp + sp * tL) / r / r + p_theta * v * c_max * u * cb / hr
                + p_l * v * st / cL / r / r + v * p_phi * ct * (sp + tt * tt * (sp - tL * cp)) / r / r - p_phi * v * c_max * u * sb / ct / hr)
        o[7] = -(p_L * ct * sp / r + p_l * st / (r * cL) - p_h * ct * cp
                 + p_theta * (c_max * u * cb + g / v / v * st * cp - ft * sa * cb / mass / v / v + st * (cp + sp * tL) / r)
                 + p_phi * (-c_max * u * sb / ct + g / v / v * sp / ct + ft * sa * sb / ct / mass / v / v + ct * (sp + tt * tt * (sp - tL * cp)) / r)
                 - p_v * 2 * (d + eta * c_max * u * u) * v)
        o[8] = (-v * (-p_L * st * sp / r + p_l * ct / (r * cL) + p_h * st * cp)
                - g * (-p_theta * ct * cp / v - p_phi * sp * tt / (v * ct) - p_v * st * cp)
                - p_theta * v * ct * (cp + sp * tL) / r + p_phi * v * st * (sp + tt * tt * (sp - tL * cp)) / r
                - p_phi * v * ct * (2 * tt * (1 + tt * tt) * (sp - tL * cp)) / r
                - p_phi * (-v * c_max * u * sb - ft * sa * sb / mass / v) * tt / ct)
        o[9] = (-v * (p_h * ct * sp + p_L * ct * cp / r)
                - g * (p_theta * st * sp / v - p_phi * cp / (v * ct) - p_v * ct * sp)
                - p_theta * (v * st * (-sp + cp * tL) / r)
                - p_phi * v * ct * (cp + tt * tt * (cp + tL * sp)) / r)
        o[10] = -p_l * v * st * tL / cL / r - v * (1 + tL * tL) * (p_theta * st * sp - p_phi * ct * cp * tt * tt) / r
    o[11] = K.lift(0.0)
    return o, [u, beta]


def hamiltonian(K, P, chart, stage, t, X, neg0=False):
    """Hamiltonian_1 / Hamiltonian_2."""
    c, s1, c1, s2, c2, u, beta, sb, cb, sa, ca = _terms(K, P, chart, stage, t, X, neg0)
    v, L = X[1], X[4]
    p_h, p_v, p_a1, p_a2, p_L, p_l = X[6:12]
    mass, c_max, d, r, g, ft, eta = c["mass"], c["c_max"], c["d"], c["r"], c["g"], c["ft"], P[ETA]
    cL, tL = K.cos(L), K.tan(L)
    if chart == 1:
        sg, cg, sc, cc, p_gamma, p_chi = s1, c1, s2, c2, p_a1, p_a2
        return (p_L * v * cg * cc / r
                + p_l * v * cg * sc / cL / r
                + p_h * v * sg
                + p_gamma * (v * c_max * u * cb - g / v * cg + ft * sa * cb / mass / v + v * cg / r)
                + p_chi * (v * c_max * u * sb / cg + ft * sa * sb / cg / mass / v + v * cg * tL * sc / r)
                - p_v * ((d + eta * c_max * u * u) * v * v + g * sg - ft * ca / mass)
                + P[MUC] * u * u / 2)
    st, ct, sp, cp, p_theta, p_phi = s1, c1, s2, c2, p_a1, p_a2
    tt = K.tan(X[2])
    return (p_L * v * ct * sp / r
            + p_l * v * st / (r * cL)
            - p_h * v * ct * cp
            + p_theta * (v * c_max * u * cb + v * st * (cp + sp * tL) / r + (ft * sa * cb / (mass * v) - g * st * cp / v))
            + p_phi * (-v * c_max * u * sb / ct + v * ct * (sp + tt * tt * (sp - tL * cp)) / r - (ft * sa * sb / (mass * v * ct) + g * sp / (v * ct)))
            - p_v * ((d + eta * c_max * u * u) * v * v - g * ct * cp - ft * ca / mass)
            + P[MUC] * u * u / 2)


def rhs_fast(K, P, chart, stage, t, X, neg0=False):
    """InterceptorT<true>::rhs_fast.  Returns Xdot[12]."""
    chart1 = chart == 1
    mutation = _mut(K)
    v, L = X[1], X[4]
    p_h, p_v, p_a1, p_a2, p_L, p_l = X[6:12]
    eta, alpha_max = P[ETA], P[ALPHA_MAX]
    c = common(K, P, stage, t, X[0], rcp=True, exp=getattr(K, "exp_lib", K.exp))
    mass, im, ihr, c_max, d, ir, g, ft = c["mass"], c["im"], c["ihr"], c["c_max"], c["d"], c["ir"], c["g"], c["ft"]
    iv = K.rcp(v)
    s1, c1 = _sincos_fast(K, X[2])
    s2, c2 = _sincos_fast(K, X[3])
    sL, cL = _sincos_fast(K, L)
    ic1, icL = K.rcp(c1), K.rcp(cL)
    tL = sL * icL
    by = p_a2 if (chart1 or mutation == "sb_unsigned") else -p_a2
    bx = p_a1 * c1
    b2 = bx * bx + by * by
    cb, sb = K.lift(1.0), K.lift(0.0)
    in_range = K.cmp("b2-lo", b2 - B2_LO, ">") and K.cmp("hi-b2", B2_HI - b2, ">")
    if not in_range and not getattr(K, "no_b2_guard", False):
        # not comfortably normal (or zero): the pair rescaled by an exact power of two, towards 1
        big = K.value(abs(bx)) > 1 or K.value(abs(by)) > 1
        k = 1.0 / B2_SCALE if big else B2_SCALE
        bx, by = bx * k, by * k
        b2 = bx * bx + by * by
    if K.cmp("b2>0", b2, ">"):
        ib = K.rsqrt(b2)
        cb, sb = bx * ib, by * ib
    W = v * c_max + ft * alpha_max * im * iv
    num = p_a1 * cb * W + (p_a2 if chart1 else -p_a2) * sb * ic1 * W
    den = p_v * (2 * eta * c_max * v * v + ft * alpha_max * alpha_max * im) - P[MUC]
    u = num / den
    if K.cmp("|u|-u_max", abs(u) - P[UMAX], ">"):
        u = K.copysign(P[UMAX], u)
    sa, ca = _sincos_fast(K, alpha_max * u)

    Kd = d + eta * c_max * u * u
    vr = v * ir
    An = ft * sa * im * iv
    Qt = v * c_max * u + An
    Kv2 = Kd * v * v
    o = [None] * 12
    if chart1:
        sg, cg, sc, cc, p_gamma, p_chi, icg = s1, c1, s2, c2, p_a1, p_a2, ic1
        vrcg = vr * cg
        lat = p_L * cc + p_l * sc * icL
        o[0] = v * sg
        o[1] = -Kv2 - g * sg + ft * ca * im
        o[2] = Qt * cb - g * iv * cg + vrcg
        o[3] = Qt * sb * icg + vrcg * tL * sc
        o[4] = vrcg * cc
        o[5] = vrcg * sc * icL
        o[6] = (-p_v * ihr * Kv2 - 2 * g * ir * (p_gamma * iv * cg + p_v * sg)
                + ir * (vrcg * (lat + p_gamma + p_chi * tL * sc))
                + ihr * v * c_max * u * (p_gamma * cb + p_chi * sb * icg))
        o[7] = -(ir * cg * lat + p_h * sg
                 + p_gamma * (c_max * u * cb + g * iv * iv * cg - An * iv * cb + cg * ir)
                 + p_chi * ((c_max * u - An * iv) * sb * icg + cg * tL * sc * ir)
                 - 2 * p_v * Kd * v)
        o[8] = (vr * sg * (lat + p_gamma + p_chi * tL * sc) - v * p_h * cg
                - g * (p_gamma * iv * sg - p_v * cg)
                - p_chi * Qt * sb * sg * icg * icg)
        o[9] = vrcg * (p_L * sc - p_l * cc * icL - p_chi * tL * cc)
        o[10] = -vrcg * sc * (p_l * sL * icL * icL + p_chi * (1 + tL * tL))
    else:
        st, ct, sp, cp, p_theta, p_phi, ict = s1, c1, s2, c2, p_a1, p_a2, ic1
        tt = st * ict
        tt2 = tt * tt
        A = cp + sp * tL
        B = sp + tt2 * (sp - tL * cp)
        givt = g * iv
        o[0] = -v * ct * cp
        o[1] = -Kv2 + g * ct * cp + ft * ca * im
        o[2] = Qt * cb + vr * st * A - givt * st * cp
        o[3] = -Qt * sb * ict + vr * ct * B - givt * sp * ict
        o[4] = vr * ct * sp
        o[5] = vr * st * icL
        o[6] = (-p_v * ihr * Kv2 - 2 * g * ir * (iv * (p_theta * st * cp + p_phi * sp * ict) - p_v * ct * cp)
                + ir * vr * (p_L * ct * sp + p_theta * st * A + p_l * st * icL + p_phi * ct * B)
                + ihr * v * c_max * u * (p_theta * cb - p_phi * sb * ict))
        o[7] = -(ir * (p_L * ct * sp + p_l * st * icL) - p_h * ct * cp
                 + p_theta * (c_max * u * cb + givt * iv * st * cp - An * iv * cb + st * A * ir)
                 + p_phi * ((-c_max * u + An * iv) * sb * ict + givt * iv * sp * ict + ct * B * ir)
                 - 2 * p_v * Kd * v)
        steep = (1 if mutation == "tan2_dropped" else 1 + tt2)
        o[8] = (-v * (-p_L * st * sp * ir + p_l * ct * ir * icL + p_h * st * cp)
                + givt * (p_theta * ct * cp + p_phi * sp * tt * ict) + g * p_v * st * cp
                - p_theta * vr * ct * A + p_phi * vr * st * B
                - p_phi * vr * ct * (2 * tt * steep * (sp - tL * cp))
                + p_phi * Qt * sb * tt * ict)
        o[9] = (-v * (p_h * ct * sp + p_L * ct * cp * ir)
                - givt * (p_theta * st * sp - p_phi * cp * ict) + g * p_v * ct * sp
                - p_theta * vr * st * (-sp + cp * tL)
                - p_phi * vr * ct * (cp + tt2 * (cp + tL * sp)))
        o[10] = -p_l * vr * st * tL * icL - vr * (1 + tL * tL) * (p_theta * st * sp - p_phi * ct * cp * tt2)
    o[11] = K.lift(0.0)
    return o


# ---- chart change ----------------------------------------------------------------------------------------------------------

def _zeros(K):
    return [[K.lift(0.0) for _ in range(6)] for _ in range(6)]


def jac_chart1(K, r, v, L, l, gamma, chi):
    cL, sL, cl, sl, cg, sg, cc, sc = K.cos(L), K.sin(L), K.cos(l), K.sin(l), K.cos(gamma), K.sin(gamma), K.cos(chi), K.sin(chi)
    J = _zeros(K)
    J[0][0] = cL * cl; J[1][0] = -r * sL * cl; J[2][0] = -r * cL * sl
    J[0][1] = cL * sl; J[1][1] = -r * sL * sl; J[2][1] = r * cL * cl
    J[0][2] = sL;      J[1][2] = r * cL
    J[1][3] = (-cL * cl * cg * cc - sL * cl * sg) * v
    J[2][3] = (sL * sl * cg * cc - cl * cg * sc - cL * sl * sg) * v
    J[3][3] = (sL * cl * sg * cc + sl * sg * sc + cL * cl * cg) * v
    J[4][3] = (sL * cl * cg * sc - sl * cg * cc) * v
    J[5][3] = (-sL * cl * cg * cc - sl * cg * sc + cL * cl * sg) * v
    J[1][4] = (-cL * sl * cg * cc - sL * sl * sg) * v
    J[2][4] = (-sL * cl * cg * cc - sl * cg * sc + cL * cl * sg) * v
    J[3][4] = (sL * sl * sg * cc - cl * sg * sc + cL * sl * cg) * v
    J[4][4] = (sL * sl * cg * sc + cl * cg * cc) * v
    J[5][4] = (-sL * sl * cg * cc + cl * cg * sc + cL * sl * sg) * v
    J[1][5] = (-sL * cg * cc + cL * sg) * v
    J[3][5] = (-cL * sg * cc + sL * cg) * v
    J[4][5] = -cL * cg * sc * v
    J[5][5] = (cL * cg * cc + sL * sg) * v
    return J


def jac_chart2(K, r, v, L, l, theta, phi):
    cL, sL, cl, sl, ct, st, cp, sp = K.cos(L), K.sin(L), K.cos(l), K.sin(l), K.cos(theta), K.sin(theta), K.cos(phi), K.sin(phi)
    J = _zeros(K)
    J[0][0] = cL * cl; J[1][0] = -r * sL * cl; J[2][0] = -r * cL * sl
    J[0][1] = cL * sl; J[1][1] = -r * sL * sl; J[2][1] = r * cL * cl
    J[0][2] = sL;      J[1][2] = r * cL
    J[1][3] = (-cL * cl * ct * sp + sL * cl * ct * cp) * v
    J[2][3] = (sL * sl * ct * sp - cl * st + cL * sl * ct * cp) * v
    J[3][3] = (sL * cl * st * sp - sl * ct + cL * cl * st * cp) * v
    J[4][3] = (-sL * cl * ct * cp + cL * cl * ct * sp) * v
    J[5][3] = (-sL * cl * ct * sp - sl * st - cL * cl * ct * cp) * v
    J[1][4] = (-cL * sl * ct * sp + sL * sl * ct * cp) * v
    J[2][4] = (-sL * cl * ct * sp - sl * st - cL * cl * ct * cp) * v
    J[3][4] = (sL * sl * st * sp + cl * ct + cL * sl * st * cp) * v
    J[4][4] = (-sL * sl * ct * cp + cL * sl * ct * sp) * v
    J[5][4] = (-sL * sl * ct * sp + cl * st - cL * sl * ct * cp) * v
    J[1][5] = (-sL * ct * sp - cL * ct * cp) * v
    J[3][5] = (-cL * st * sp + sL * st * cp) * v
    J[4][5] = (cL * ct * cp + sL * ct * sp) * v
    J[5][5] = (cL * ct * sp - sL * ct * cp) * v
    if _mut(K) == "jac2_swap":
        J[4][4], J[4][5] = J[4][5], J[4][4]
    return J


def lu6_solve(K, A, y, tag=""):
    """y <- A^-1 y by partial-pivot LU, the pivot the first largest |entry| of the column; sums left to right."""
    A = [row[:] for row in A]
    y = y[:]
    for k in range(6):
        cand = sorted(range(k, 6), key=lambda i: (-K.value(abs(A[i][k])), i))
        piv = cand[0]
        if len(cand) > 1:
            name = "pivot%d%s" % (k, tag)
            K.margins[name] = abs(A[cand[0]][k]) - abs(A[cand[1]][k])
            if name in K.flip:
                piv = cand[1]
        if piv != k:
            A[k], A[piv] = A[piv], A[k]
            y[k], y[piv] = y[piv], y[k]
        if K.value(A[k][k]) != 0:
            for i in range(k + 1, 6):
                A[i][k] = A[i][k] / A[k][k]
        for i in range(k + 1, 6):
            if K.value(A[i][k]) == 0 and _exact_zero(A[i][k]):
                continue                                                  # a structural zero: a - 0 * b is a, exactly
            for j in range(k + 1, 6):
                A[i][j] = A[i][j] - A[i][k] * A[k][j]
    for i in range(1, 6):
        for j in range(i):
            if not (K.value(A[i][j]) == 0 and _exact_zero(A[i][j])):
                y[i] = y[i] - A[i][j] * y[j]
    for i in range(5, -1, -1):
        for j in range(i + 1, 6):
            if not (K.value(A[i][j]) == 0 and _exact_zero(A[i][j])):
                y[i] = y[i] - A[i][j] * y[j]
        y[i] = y[i] / A[i][i]
    return y


def _exact_zero(q):
    if isinstance(q, Tracked):
        return q.e == 0
    return getattr(q, "exact", True)                                      # dopri5_reference.Affine says so itself; a plain number is exact


def new_angles(K, from1, a1, a2, raw_a1, tag=""):
    """The other chart's angle pair.  raw_a1: the double a1 is (None inside a trajectory, where it is computed)."""
    L = K.lift
    hp = L(PI / 2.0)
    if from1:
        at_plus, at_minus = (L(0.0), L(-PI)), (L(0.0), L(0.0))
    else:
        at_plus, at_minus = (L(0.0), hp), (L(0.0), L(-PI / 2.0))
    if raw_a1 is not None:
        if raw_a1 == PI / 2.0:
            return at_plus
        if raw_a1 == -PI / 2.0:
            return at_minus
    else:                                                                 # on computed values the equality is a decision like any other
        if K.value(a1 - hp) == 0:
            return at_plus
        if K.value(a1 + hp) == 0:
            return at_minus
    s1, c1, s2, c2 = K.sin(a1), K.cos(a1), K.sin(a2), K.cos(a2)
    if from1:
        n1 = K.acos(K.sqrt(s1 * s1 + c1 * c1 * c2 * c2))
        if K.cmp("c1*s2<0" + tag, c1 * s2, "<"):
            n1 = -n1
        cn = K.cos(n1)
        key, sel, arg = c1 * c2 / cn, s1 / cn, -s1 / cn
        zero_if, pi_if = "<", ">"
    else:
        n1 = K.acos(K.sqrt(s1 * s1 + c1 * c1 * s2 * s2))
        if K.cmp("c1*c2>0" + tag, c1 * c2, ">"):
            n1 = -n1
        cn = K.cos(n1)
        key, sel, arg = s1 / cn, s2 * c1 / cn, s2 * c1 / cn
        zero_if, pi_if = ">", "<"
    if K.cmp("|key|-eps" + tag, abs(key) - EPS, "<"):
        if K.cmp("sel:zero" + tag, sel, zero_if):
            return n1, L(0.0)
        if K.cmp("sel:pi" + tag, sel, pi_if):
            return n1, L(-PI)
    if K.cmp("key>0" + tag, key, ">"):
        return n1, K.acos(arg)
    return n1, -K.acos(arg)


def change_chart(K, P, from1, X, raw_a1=None, tag=""):
    """ConversionState12 (from1) / ConversionState21: the state in the other chart."""
    v, a1, a2, L, l = X[1], X[2], X[3], X[4], X[5]
    r = X[0] + P[REARTH]
    n1, n2 = new_angles(K, from1, a1, a2, raw_a1, tag)
    if from1:
        Jf, Jt = jac_chart1(K, r, v, L, l, a1, a2), jac_chart2(K, r, v, L, l, n1, n2)
    else:
        Jf, Jt = jac_chart2(K, r, v, L, l, a1, a2), jac_chart1(K, r, v, L, l, n1, n2)
    p = lu6_solve(K, Jf, [X[6], X[10], X[11], X[8], X[9], X[7]], tag)
    q = []
    for i in range(6):
        acc = Jt[i][0] * p[0]
        for j in range(1, 6):
            if K.value(Jt[i][j]) == 0 and _exact_zero(Jt[i][j]):
                continue
            acc = acc + Jt[i][j] * p[j]
        q.append(acc)
    out = list(X)
    out[2], out[3] = n1, n2
    out[6], out[7], out[8], out[9], out[10], out[11] = q[0], q[5], q[3], q[4], q[1], q[2]
    return out


def set_chart(K, P, chart, X, tag=""):
    if K.cmp("|cos a1|-limit" + tag, abs(K.cos(X[2])) - P[CHART_LIMIT], ">="):
        return chart, X
    return (2 if chart == 1 else 1), change_chart(K, P, chart == 1, X, None, tag)


def rk4_step(K, P, chart, stage, t, X, step, rhs=None):
    """odeTools::RK4 (the function-pointer overload): X + h/6 (F1 + (F4 + 2 (F2 + F3)))."""
    f = rhs or (lambda tt, Y: rhs_ref(K, P, chart, stage, tt, Y)[0])
    F1 = f(t, X)
    F2 = f(t + step / 2.0, [a + step / 2.0 * k for a, k in zip(X, F1)])
    F3 = f(t + step / 2.0, [a + step / 2.0 * k for a, k in zip(X, F2)])
    F4 = f(t + step, [a + step * k for a, k in zip(X, F3)])
    return [a + step / 6.0 * (k1 + (k4 + 2.0 * (k2 + k3))) for a, k1, k2, k3, k4 in zip(X, F1, F2, F3, F4)]


def compute_traj(K, P, step_nbr, t0, tf, X, form="ref"):
    """interceptor::ComputeTraj over ModelInt on the kit's numbers.  t0, tf are doubles and so are t1, the step and the times of the
    steps (t += dt), formed in float64 as every implementation forms them: the recurrence is the same in every kit, only the
    arithmetic of the right-hand side and of the updates differs.  Returns (Xf, rows) with rows[k] = (X, chart, stage) as the dense
    entry point stores them: stage start, after every step, and the handed-back row."""
    chart = 1
    t0, tf = float(t0), float(tf)
    t1 = float(F64(float(K.value(P[PROP]))) / F64(float(K.value(P[Q]))))
    two = t0 < t1 and tf > t1
    stage = 1 if t0 < t1 else 0
    fn = rhs_fast if form == "fast" else (lambda *a: rhs_ref(*a)[0])
    rows = []
    n = 0
    for ph in range(2 if two else 1):
        ta = t0 if ph == 0 else t1
        tb = t1 if (two and ph == 0) else tf
        if ph == 1:
            stage = 0
        rows.append((X, chart, stage))
        dt = float(F64(tb - ta) / F64(step_nbr))
        t = ta
        for _ in range(step_nbr):
            chart, X = set_chart(K, P, chart, X, ":%d" % n)
            n += 1
            X = rk4_step(K, P, chart, stage, K.lift(t), X, K.lift(dt), rhs=lambda tt, Y: fn(K, P, chart, stage, tt, Y))
            t = float(F64(t) + F64(dt))
            rows.append((X, chart, stage))
    if chart == 2 and _mut(K) != "no_handback":
        X = change_chart(K, P, False, X, None, ":back")
    rows.append((X, chart, stage))
    return X, rows


# ---- running the restatements -----------------------------------------------------------------------------------------------

class FastTrackedKit(TrackedKit):
    """The throughput translation unit: exp_glibc in common() is not used by rhs_fast, which calls the library's exp."""

    def exp_lib(self, a):
        return TrackedKit(c_exp=C_EXP_LIB).exp(a)


def _lift(K, P, X):
    return [K.lift(p) for p in P], [K.lift(q) for q in X]


def _neg0(X):
    return bool(np.signbit(X[9]))


def emulate_rhs(form, P, chart, stage, t, X, **kit):
    """One restatement in numpy.float64, one rounding per operation (the short sincos with its fused operations exactly): (Xdot[12],
    [u, beta], H); control and Hamiltonian are the reference-order text in either form."""
    K = F64Kit(**{k: v for k, v in kit.items() if k != "no_b2_guard"})
    K.no_b2_guard = kit.get("no_b2_guard", False)
    with np.errstate(all="ignore"):
        Pk, Xk = _lift(K, P, X)
        d_ref, ub = rhs_ref(K, Pk, chart, stage, K.lift(t), Xk, _neg0(X))
        d = rhs_fast(K, Pk, chart, stage, K.lift(t), Xk, _neg0(X)) if form == "fast" else d_ref
        H = hamiltonian(K, Pk, chart, stage, K.lift(t), Xk, _neg0(X))
    return np.array(d, dtype=F64), np.array(ub, dtype=F64), F64(H)


def emulate_chart(P, from1, X, flip=(), **kit):
    K = F64Kit(flip=flip, **kit)
    with np.errstate(all="ignore"):
        Pk, Xk = _lift(K, P, X)
        return np.array(change_chart(K, Pk, from1, Xk, float(X[2])), dtype=F64)


def evaluate_row(P, chart, stage, t, X, flip=()):
    """One right-hand-side row through both restatements on Tracked numbers: value[12], B_ref[12], B_fast[12], u[2], B_u[2], H, B_H,
    decidable, undecided."""
    Kr, Kf = TrackedKit(flip), FastTrackedKit(flip)
    Pr, Xr = _lift(Kr, P, X)
    d_ref, ub = rhs_ref(Kr, Pr, chart, stage, Kr.lift(t), Xr, _neg0(X))
    Kh = TrackedKit(flip)
    H = hamiltonian(Kh, Pr, chart, stage, Kh.lift(t), Xr, _neg0(X))
    Pf, Xf = _lift(Kf, P, X)
    d_fast = rhs_fast(Kf, Pf, chart, stage, Kf.lift(t), Xf, _neg0(X))
    out = {}
    tiny = mpf(2) ** -150
    assert flip or all(abs(a.v - b.v) <= tiny * (abs(a.v) + abs(b.v)) + (a.e + b.e) * tiny + mpf(2) ** -1200
                       for a, b in zip(d_ref, d_fast)), "the two restatements disagree"
    rebased = [Tracked(a.v, b.e + abs(a.v - b.v)) for a, b in zip(d_ref, d_fast)]
    out["value"], out["B_ref"] = fr._pin(d_ref)
    out["B_fast"] = fr._pin(rebased)[1]
    out["u"], out["B_u"] = fr._pin(ub)
    h, bh = fr._pin([H])
    out["H"], out["B_H"] = h[0], bh[0]
    out["undecided"] = sorted(set(Kr.undecided()) | set(Kf.undecided()) | set(Kh.undecided()))
    out["decidable"] = not out["undecided"]
    out["finite"] = all(mpmath.isfinite(q.v) and mpmath.isfinite(q.e) for q in d_ref + d_fast + ub + [H])
    return out


def evaluate_chart(P, from1, X, flip=()):
    """The chart change of the doubles X on Tracked numbers: value[12], B[12] (reference order; shared by both flavours), decidable,
    undecided."""
    K = TrackedKit(flip)
    Pk, Xk = _lift(K, P, X)
    val, B = fr._pin(change_chart(K, Pk, from1, Xk, float(X[2])))
    return {"value": val, "B": B, "undecided": K.undecided(), "decidable": K.decidable()}


def traj_mpf(P, step_nbr, t0, tf, X0):
    """ComputeTraj in mpf, every decision on exact values.  Returns (Xf as doubles, the smallest chart-limit margin met, [(chart,
    stage)] of the rows)."""
    K = MpfKit()
    Pk, Xk = _lift(K, P, X0)
    Xf, rows = compute_traj(K, Pk, step_nbr, t0, tf, Xk)
    limit = min([abs(float(m)) for n, m in K.margins.items() if n.startswith("|cos a1|-limit")] or [np.inf])
    return np.array([float(q) for q in Xf]), Xf, limit, [(c, s) for _, c, s in rows]


def emulate_traj(P, step_nbr, t0, tf, X0, form="ref", **kit):
    K = F64Kit(**kit)
    with np.errstate(all="ignore"):
        Pk, Xk = _lift(K, P, X0)
        Xf, rows = compute_traj(K, Pk, step_nbr, t0, tf, Xk, form)
    return np.array(Xf, dtype=F64), [np.array(r[0], dtype=F64) for r in rows]
