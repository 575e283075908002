"""High-precision values and derived rounding bounds for the Goddard and covid19 right-hand sides (helper of
test_fast_pin_cpu.py, test_gpu_fast_pin.py and golden/make_fast_golden.py, not a test).

The right-hand sides are restated ONCE over a generic number type ("kit"), in two forms:

  *_ref   the reference operation order, expression by expression as oracle/socp_oracle.c writes it;
  *_fast  the throughput flavour's structure as socp_amd/csrc/models_fast.hpp describes it (three inverse square roots, one
          reciprocal, one exp, the factored gravity-gradient block; covid19: three reciprocals of constants, one shared flux).

The same text runs on
  MpfKit      mpmath numbers (the value),
  TrackedKit  Tracked(value, err): first-order running error analysis (Higham, Accuracy and Stability, 3.3) -- the bound,
  F64Kit      numpy.float64, one rounding per operation -- a CPU emulation (and the carrier of the instrument's mutation checks).

Error model of Tracked (u = 2^-53, res the exact result, ea / eb the operands' bounds):
    a +- b   ea + eb + u|res|                          a * b    |a| eb + |b| ea + u|res|
    a / b    (ea + |res| eb)/|b| + u|res|              sqrt a   ea / (2 sqrt a) + u|res|
    exp a    |res| ea + C_EXP u|res|                   1/a, 1/sqrt a as the fast flavour forms them: same propagation, C_RCP, C_RSQ
    tanh a   (1 - res^2) ea + C_TANH u|res|            (a kit built with c_exp = C_EXP_LIB charges the library's exp that budget)
    sin a    |cos a| ea + C_SIN u|res|                 cos a    |sin a| ea + C_COS u|res|
    tan a    (1 + res^2) ea + C_TAN u|res|             atan2(y, x)   (|x| ey + |y| ex)/(x^2 + y^2) + C_ATAN2 u|res|
    acos a   the enclosure max |acos(a -+ ea) - acos a| (arguments clamped to [-1, 1]) + C_ACOS u|res|: to first order that is
             ea / sqrt(1 - a^2), and like it it grows without limit relative to ea as |a| -> 1 (sqrt(2 ea) at |a| = 1), but it stays
             a bound there, which the first-order term is not
    copysign(a, b)   |a| with the sign of b's exact value; a's error (the caller records the sign of b as a decision where it matters)
Within second_order_products() a product also carries ea eb: where BOTH factors vanish to the working precision (vtolUAV's 1 - tanh h
far from a box) the first-order terms are zero and that term is all that is left.  Goddard and covid19 do not use it.
Inputs and parameters carry err = 0.  C_EXP = C_RCP = C_RSQ = 2: the budget the comments of models_fast.hpp claim, doubled.  A fused
multiply-add is counted as a product and a sum (two roundings): an upper bound of what contraction does.  Gradual underflow is in
the model the standard way (Higham 2.8): a product, quotient, root or exp whose result is subnormal adds 2^-1075 absolute; an exp
whose result is subnormal adds 4 * 2^-1074 instead, which propagates to each component times the component's sensitivity to it.

Every branch decision is taken on the exact value and recorded with the Tracked error of its margin.  A row is DECIDABLE when every
margin exceeds 4x its error (a margin whose error is zero, e.g. t == sw0 compared exactly, is decidable: both flavours compare the
same two doubles).  Near a kink the flavours may take different branches; `flip` forces the other branch of named decisions.
"""
import contextlib

import numpy as np

try:
    import mpmath
    from mpmath import mpf
    HAVE_MPMATH = True
    mpmath.mp.prec = 240
except ImportError:                                   # the GPU tests read the fixture only
    mpmath = None
    mpf = None
    HAVE_MPMATH = False

F64 = np.float64
C_EXP = C_RCP = C_RSQ = 2
# library calls whose accuracy the project does not control (vtolUAV: the device library's tanh and exp): the published OpenCL
# full-profile limits the device library is built to, tanh <= 5 ulp and exp <= 3 ulp, with ulp = 2u.  Taken from the specification,
# not measured.
C_TANH, C_EXP_LIB = 10, 6
# the interceptor's library calls, same source (OpenCL full profile: sin, cos, acos <= 4 ulp, tan <= 5 ulp, atan2 <= 6 ulp; ulp = 2u).
# Taken from the specification, not measured.
C_SIN = C_COS = C_ACOS = 8
C_TAN = 10
C_ATAN2 = 12
DECIDE_FACTOR = 4

if HAVE_MPMATH:
    U = mpf(2) ** -53
    ETA = mpf(2) ** -1075
    TINY = mpf(2) ** -1022
    EXP_FLOOR = 4 * mpf(2) ** -1074


class Tracked:
    """value (mpf, the exact result of the expression so far) and err (mpf, first-order bound of |computed - value|)."""
    __slots__ = ("v", "e")
    second_order = False                              # second_order_products() sets it

    def __init__(self, v, e=0):
        self.v = v if isinstance(v, mpf) else mpf(float(v))
        self.e = e if isinstance(e, mpf) else mpf(e)

    @staticmethod
    def lift(x):
        return x if isinstance(x, Tracked) else Tracked(x)

    @staticmethod
    def _rounded(res, prop, c=1, underflow=True):
        a = abs(res)
        e = prop + c * U * a
        if underflow and 0 < a < TINY:
            e += ETA
        return Tracked(res, e)

    def __neg__(self):
        return Tracked(-self.v, self.e)

    def __abs__(self):
        return Tracked(abs(self.v), self.e)

    def __add__(self, o):
        o = Tracked.lift(o)
        return Tracked._rounded(self.v + o.v, self.e + o.e, underflow=False)

    __radd__ = __add__

    def __sub__(self, o):
        o = Tracked.lift(o)
        return Tracked._rounded(self.v - o.v, self.e + o.e, underflow=False)

    def __rsub__(self, o):
        return Tracked.lift(o) - self

    def __mul__(self, o):
        o = Tracked.lift(o)
        prop = abs(self.v) * o.e + abs(o.v) * self.e
        if Tracked.second_order:
            prop += self.e * o.e
        return Tracked._rounded(self.v * o.v, prop)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Tracked.lift(o)
        res = self.v / o.v
        return Tracked._rounded(res, (self.e + abs(res) * o.e) / abs(o.v))

    def __rtruediv__(self, o):
        return Tracked.lift(o) / self


@contextlib.contextmanager
def second_order_products():
    """Tracked products carry |a| eb + |b| ea + ea eb (the exact bound of a product of two perturbed factors) while this is open."""
    before, Tracked.second_order = Tracked.second_order, True
    try:
        yield
    finally:
        Tracked.second_order = before


class _Kit:
    """Number type + the decisions taken.  margins[name] = the margin as the kit's number."""

    def __init__(self, flip=()):
        self.flip = frozenset(flip)
        self.margins = {}

    def cmp(self, name, m, op):
        v = self.value(m)
        d = {"<": v < 0, "<=": v <= 0, ">": v > 0, ">=": v >= 0}[op]
        self.margins[name] = m
        return (not d) if name in self.flip else bool(d)

    def cmp_exact(self, name, a, b, op):
        """a op b for two INPUTS (doubles, no error): both flavours compare the same two doubles, so the margin's error is zero."""
        m = self.exact_diff(a, b)
        v = self.value(m)
        self.margins[name] = m
        return bool({"<": v < 0, ">": v > 0, "==": v == 0}[op])


class MpfKit(_Kit):
    def lift(self, x):
        return mpf(float(x))

    def value(self, x):
        return x

    def exact_diff(self, a, b):
        return a - b

    sqrt = staticmethod(lambda x: mpmath.sqrt(x))
    exp = staticmethod(lambda x: mpmath.exp(x))
    tanh = staticmethod(lambda x: mpmath.tanh(x))
    rcp = staticmethod(lambda x: 1 / x)
    rsqrt = staticmethod(lambda x: 1 / mpmath.sqrt(x))
    sin = staticmethod(lambda x: mpmath.sin(x))
    cos = staticmethod(lambda x: mpmath.cos(x))
    tan = staticmethod(lambda x: mpmath.tan(x))
    acos = staticmethod(lambda x: mpmath.acos(_clamp1(x)))
    copysign = staticmethod(lambda a, b: abs(a) if b >= 0 else -abs(a))

    @staticmethod
    def atan2(y, x, y_negative_zero=False):
        return _atan2_mpf(y, x, y_negative_zero)


def _clamp1(x):
    return max(mpf(-1), min(mpf(1), x))


def _atan2_mpf(y, x, y_negative_zero):
    """atan2 with the sign of a zero y, which mpf does not carry: atan2(-0.0, x < 0) = -pi."""
    if y == 0 and x == 0:
        return mpf(0)
    if y == 0 and x < 0:
        return -mpmath.pi if y_negative_zero else +mpmath.pi
    return mpmath.atan2(y, x)


class TrackedKit(_Kit):
    def __init__(self, flip=(), c_exp=C_EXP):
        super().__init__(flip)
        self.c_exp = c_exp

    def lift(self, x):
        return Tracked(x)

    def value(self, x):
        return x.v

    def exact_diff(self, a, b):
        assert a.e == 0 and b.e == 0
        return Tracked(a.v - b.v, 0)

    @staticmethod
    def sqrt(a):
        res = mpmath.sqrt(a.v)
        return Tracked._rounded(res, a.e / (2 * res) if a.e else mpf(0))

    def exp(self, a):
        res = mpmath.exp(a.v)
        e = res * a.e + self.c_exp * U * res
        if res < TINY:
            e += EXP_FLOOR
        return Tracked(res, e)

    @staticmethod
    def tanh(a):
        res = mpmath.tanh(a.v)
        return Tracked(res, (1 - res * res) * a.e + C_TANH * U * abs(res))

    @staticmethod
    def rcp(a):
        res = 1 / a.v
        return Tracked._rounded(res, a.e * res * res, c=C_RCP)

    @staticmethod
    def rsqrt(a):
        res = 1 / mpmath.sqrt(a.v)
        return Tracked._rounded(res, a.e * abs(res) / (2 * abs(a.v)) if a.e else mpf(0), c=C_RSQ)

    @staticmethod
    def sin(a):
        res = mpmath.sin(a.v)
        return Tracked(res, abs(mpmath.cos(a.v)) * a.e + C_SIN * U * abs(res))

    @staticmethod
    def cos(a):
        res = mpmath.cos(a.v)
        return Tracked(res, abs(mpmath.sin(a.v)) * a.e + C_COS * U * abs(res))

    @staticmethod
    def tan(a):
        res = mpmath.tan(a.v)
        return Tracked(res, (1 + res * res) * a.e + C_TAN * U * abs(res))

    @staticmethod
    def atan2(y, x, y_negative_zero=False):
        res = _atan2_mpf(y.v, x.v, y_negative_zero)
        n2 = x.v * x.v + y.v * y.v
        prop = (abs(x.v) * y.e + abs(y.v) * x.e) / n2 if n2 else mpf(0)
        return Tracked(res, prop + C_ATAN2 * U * abs(res))

    @staticmethod
    def acos(a):
        v = _clamp1(a.v)
        res = mpmath.acos(v)
        prop = max(mpmath.acos(_clamp1(v - a.e)) - res, res - mpmath.acos(_clamp1(v + a.e))) if a.e else mpf(0)
        return Tracked(res, prop + C_ACOS * U * abs(res))

    @staticmethod
    def copysign(a, b):
        return Tracked(abs(a.v) if b.v >= 0 else -abs(a.v), a.e)

    def decidable(self):
        return all(m.e == 0 or abs(m.v) > DECIDE_FACTOR * m.e for m in self.margins.values())

    def undecided(self):
        return [n for n, m in self.margins.items() if not (m.e == 0 or abs(m.v) > DECIDE_FACTOR * m.e)]


class F64Kit(_Kit):
    """numpy.float64, one rounding per operation; 1/x, 1/sqrt x and exp from numpy unless replaced (the mutation checks replace
    them); flip_gravity_gradient negates the p_v / r^3 term of the fast structure's dX[7]."""

    def __init__(self, flip=(), rcp=None, rsqrt=None, exp=None, tanh=None, flip_gravity_gradient=False, mutation=None):
        super().__init__(flip)
        self.rcp = rcp or (lambda x: F64(1.0) / x)
        self.rsqrt = rsqrt or (lambda x: F64(1.0) / np.sqrt(x))
        self.exp = exp or np.exp
        self.tanh = tanh or np.tanh
        self.flip_gravity_gradient = flip_gravity_gradient
        self.mutation = mutation                      # vtol_reference.vtol_fast: a named structural defect of the mutation checks

    def lift(self, x):
        return F64(x)

    def value(self, x):
        return x

    def exact_diff(self, a, b):
        return a - b

    sqrt = staticmethod(np.sqrt)
    sin = staticmethod(np.sin)
    cos = staticmethod(np.cos)
    tan = staticmethod(np.tan)
    acos = staticmethod(np.arccos)
    copysign = staticmethod(np.copysign)

    @staticmethod
    def atan2(y, x, y_negative_zero=False):
        return np.arctan2(y, x)                       # a float64 carries the sign of its zero itself


# ---- Goddard ----------------------------------------------------------------------------------------------------------------
# parameter block order: C, b, KD, kr, u_max, mu1, mu2, singularControl (socp_amd.capi.GODDARD_PARAM_NAMES)

def _singular(K, P, X, r, v, g, norm_pv, E, pvdotv):
    """The closed-form singular-arc thrust bu/au (oracle/socp_oracle.c: orc_goddard_singular_control), on the given r, v, g,
    |p_v|, E = exp(-kr (r - 1)) and p_v.v -- the reference forms them by sqrt and division, the fast flavour hands over its own."""
    x, y, z, vx, vy, vz, mass = X[0:7]
    p_x, p_y, p_z, p_vx, p_vy, p_vz = X[7:13]
    C, b, KD, kr = P[0:4]
    rdotv = x*vx + y*vy + z*vz
    D = KD*E
    p_xdot = -kr*KD / mass*v*E*x / r*pvdotv + g*(p_vx*(1 - 3 * x*x / r / r) / r - p_vy * 3 * x*y / r / r / r - p_vz * 3 * x*z / r / r / r)
    p_ydot = -kr*KD / mass*v*E*y / r*pvdotv + g*(-p_vx * 3 * y*x / r / r / r + p_vy*(1 - 3 * y*y / r / r) / r - p_vz * 3 * y*z / r / r / r)
    p_zdot = -kr*KD / mass*v*E*z / r*pvdotv + g*(-p_vx * 3 * z*x / r / r / r - p_vy * 3 * z*y / r / r / r + p_vz*(1 - 3 * z*z / r / r) / r)
    p_vxdot = -p_x + KD / mass*E*(pvdotv*vx / v + p_vx*v)
    p_vydot = -p_y + KD / mass*E*(pvdotv*vy / v + p_vy*v)
    p_vzdot = -p_z + KD / mass*E*(pvdotv*vz / v + p_vz*v)
    prdotdotpv = p_xdot*p_vx + p_ydot*p_vy + p_zdot*p_vz
    prdotpvdot = p_x*p_vxdot + p_y*p_vydot + p_z*p_vzdot
    prdotpv = p_x*p_vx + p_y*p_vy + p_z*p_vz
    pvdotdotv = p_vxdot*vx + p_vydot*vy + p_vzdot*vz
    pvdotdotpv = p_vxdot*p_vx + p_vydot*p_vy + p_vzdot*p_vz
    vdotg = vx*g*x / r + vy*g*y / r + vz*g*z / r
    pvdotg = p_vx*g*x / r + p_vy*g*y / r + p_vz*g*z / r
    au = (2 * norm_pv*C / mass*pvdotv
          + 2 * pvdotv*C / mass*norm_pv
          - b / mass*(2 * pvdotv*pvdotv + norm_pv*norm_pv*v*v)
          - b / D*v*prdotpv - C / D*prdotpv / v*pvdotv / norm_pv)
    bu = (-2 * norm_pv*norm_pv*(vdotg + D / mass*v*v*v) + 2 * v*v*pvdotdotpv
          - 2 * pvdotv*(pvdotg + D / mass*v*pvdotv - pvdotdotv)
          + b / C*(2 * norm_pv*pvdotv*(vdotg + D / mass*v*v*v) + norm_pv*v*v*(pvdotg + D / mass*v*pvdotv - pvdotdotv) - v*v*pvdotv / norm_pv*pvdotdotpv)
          - mass / D*kr*rdotv / r*v*prdotpv + mass / D*prdotpv / v*(vdotg + D / mass*v*v*v) - mass / D*v*(prdotdotpv + prdotpvdot))
    return bu / au


def _alpha(K, P, sw, t, X, Switch, scale, singular):
    """The thrust magnitude of the control law and whether it saturates: (alpha, saturated).  scale(Switch) is -Switch/(2 mu2) as the
    flavour forms it; singular() the singular-arc value as the flavour forms it.  Decisions: Switch < 0, Switch + 2 mu2 u_max < 0
    (<=> alpha > u_max), t <= sw0, t <= sw1, |alpha| > u_max on a singular arc."""
    u_max, mu2, sing = P[4], P[6], P[7]
    alpha = K.lift(0.0)
    sat = False
    if K.value(mu2) > 0:
        if K.cmp("Switch", Switch, "<"):
            alpha = scale(Switch)
            sat = K.cmp("Switch+2mu2umax", Switch + 2 * mu2 * u_max, "<")
    elif K.cmp("t-sw0", t - sw[0], "<="):
        alpha = K.lift(1.0)
        sat = bool(1.0 > K.value(u_max))
    elif K.cmp("t-sw1", t - sw[1], "<="):
        if K.value(sing) < 0:
            alpha = singular()
            sat = K.cmp("|alpha|-umax", abs(alpha) - u_max, ">")
        else:
            alpha = sing
            sat = bool(abs(K.value(sing)) > K.value(u_max))
    return alpha, sat


def goddard_ref(K, P, sw, t, X):
    """Reference operation order (oracle/socp_oracle.c: goddard_control, goddard_model, goddard_hamiltonian).
    Returns (Xdot[14], u[3], H)."""
    x, y, z, vx, vy, vz, mass = X[0:7]
    p_x, p_y, p_z, p_vx, p_vy, p_vz, p_mass = X[7:14]
    C, b, KD, kr, u_max, mu1, mu2 = P[0:7]
    exp = K.exp
    r = K.sqrt(x*x + y*y + z*z)
    v = K.sqrt(vx*vx + vy*vy + vz*vz)
    pvdotv = p_vx*vx + p_vy*vy + p_vz*vz
    g = 1 / r / r
    # control
    norm_pv = K.sqrt(p_vx*p_vx + p_vy*p_vy + p_vz*p_vz)
    Switch = mu1 - b*p_mass - C / mass*norm_pv
    alpha_u, sat = _alpha(K, P, sw, t, X, Switch, lambda s: -s / 2 / mu2,
                          lambda: _singular(K, P, X, r, v, g, norm_pv, exp(-kr*(r - 1)), pvdotv))
    u = [-p_vx*alpha_u / norm_pv, -p_vy*alpha_u / norm_pv, -p_vz*alpha_u / norm_pv]
    if sat:
        norm_a = abs(alpha_u)
        u = [ui / norm_a*u_max for ui in u]
    norm_u = K.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])
    pvdotu = p_vx*u[0] + p_vy*u[1] + p_vz*u[2]

    d = [None] * 14
    d[0], d[1], d[2] = vx, vy, vz
    d[3] = -KD*v*vx*exp(-kr*(r - 1)) / mass - g*x / r + C*u[0] / mass
    d[4] = -KD*v*vy*exp(-kr*(r - 1)) / mass - g*y / r + C*u[1] / mass
    d[5] = -KD*v*vz*exp(-kr*(r - 1)) / mass - g*z / r + C*u[2] / mass
    d[6] = -b*norm_u
    d[7] = -kr*KD / mass*v*exp(-kr*(r - 1))*x / r*pvdotv + g*(p_vx*(1 - 3 * x*x / r / r) / r - p_vy * 3 * x*y / r / r / r - p_vz * 3 * x*z / r / r / r)
    d[8] = -kr*KD / mass*v*exp(-kr*(r - 1))*y / r*pvdotv + g*(-p_vx * 3 * y*x / r / r / r + p_vy*(1 - 3 * y*y / r / r) / r - p_vz * 3 * y*z / r / r / r)
    d[9] = -kr*KD / mass*v*exp(-kr*(r - 1))*z / r*pvdotv + g*(-p_vx * 3 * z*x / r / r / r - p_vy * 3 * z*y / r / r / r + p_vz*(1 - 3 * z*z / r / r) / r)
    d[10] = -p_x + KD / mass*exp(-kr*(r - 1))*(pvdotv*vx / v + p_vx*v)
    d[11] = -p_y + KD / mass*exp(-kr*(r - 1))*(pvdotv*vy / v + p_vy*v)
    d[12] = -p_z + KD / mass*exp(-kr*(r - 1))*(pvdotv*vz / v + p_vz*v)
    d[13] = -KD*exp(-kr*(r - 1)) / mass / mass*v*pvdotv + C / mass / mass*pvdotu

    H = (mu1*norm_u + mu2*norm_u*norm_u
         + p_x*vx + p_y*vy + p_z*vz
         + p_vx*(-KD*v*vx*exp(-kr*(r - 1)) / mass - g*x / r + C*u[0] / mass)
         + p_vy*(-KD*v*vy*exp(-kr*(r - 1)) / mass - g*y / r + C*u[1] / mass)
         + p_vz*(-KD*v*vz*exp(-kr*(r - 1)) / mass - g*z / r + C*u[2] / mass)
         - p_mass*b*norm_u)
    return d, u, H


def goddard_fast(K, P, sw, t, X):
    """The throughput flavour's structure (models_fast.hpp: GoddardFastT::rhs).  Returns Xdot[14]."""
    x, y, z, vx, vy, vz, mass = X[0:7]
    p_x, p_y, p_z, p_vx, p_vy, p_vz, p_mass = X[7:14]
    C, b, KD, kr, u_max, mu1, mu2 = P[0:7]
    r2 = x*x + y*y + z*z
    v2 = vx*vx + vy*vy + vz*vz
    q2 = p_vx*p_vx + p_vy*p_vy + p_vz*p_vz
    ir, iv, iq = K.rsqrt(r2), K.rsqrt(v2), K.rsqrt(q2)
    r, v, norm_pv = r2 * ir, v2 * iv, q2 * iq
    im = K.rcp(mass)
    pvdotv = p_vx*vx + p_vy*vy + p_vz*vz
    pvdotr = p_vx*x + p_vy*y + p_vz*z
    E = K.exp(-kr*(r - 1))
    ir2 = ir * ir
    ir3 = ir2 * ir

    Cm = C * im
    Switch = mu1 - b*p_mass - Cm*norm_pv
    alpha, sat = _alpha(K, P, sw, t, X, Switch, lambda s: -s * (0.5 / mu2),
                        lambda: _singular(K, P, X, r, v, ir2, norm_pv, E, pvdotv))
    if sat:
        a_eff = u_max if K.value(alpha) >= 0 else -u_max
        norm_u = u_max
    else:
        a_eff = alpha
        norm_u = abs(alpha)
    ua = -a_eff * iq
    pvdotu = -a_eff * norm_pv

    Dm = KD * E * im
    Dv = Dm * v
    Tm = Cm * ua
    d = [None] * 14
    d[0], d[1], d[2] = vx, vy, vz
    d[3] = Tm*p_vx - Dv*vx - ir3*x
    d[4] = Tm*p_vy - Dv*vy - ir3*y
    d[5] = Tm*p_vz - Dv*vz - ir3*z
    d[6] = -b*norm_u
    W = -(kr * Dv * pvdotv * ir) - 3.0 * ir3 * ir2 * pvdotr
    gx = ir3*p_vx
    if getattr(K, "flip_gravity_gradient", False):
        gx = -gx
    d[7] = W*x + gx
    d[8] = W*y + ir3*p_vy
    d[9] = W*z + ir3*p_vz
    DG = Dm * (pvdotv * iv)
    d[10] = DG*vx + (Dv*p_vx - p_x)
    d[11] = DG*vy + (Dv*p_vy - p_y)
    d[12] = DG*vz + (Dv*p_vz - p_z)
    d[13] = im * (Cm*pvdotu - Dv*pvdotv)
    return d


# ---- covid19 ----------------------------------------------------------------------------------------------------------------
# parameter block order: R0, Tinf, Tinc, N, Imax, muI, umin, umax

def covid_ref(K, P, sw, t, X):
    """Reference operation order (oracle/socp_oracle.c: covid_control, covid_model).  Returns (Xdot[8], [u], None)."""
    S, E, I, R, pS, pE, pI, pR = X
    R0, Tinf, Tinc, N, Imax, muI, umin, umax = P
    u = (pE - pS)*S*I / Tinf / N * R0
    if K.cmp("u-umin", u - umin, "<="):
        u = umin
    if K.cmp("u-umax", u - umax, ">="):
        u = umax
    Rt = R0 * (1 - u)
    Ipen = K.lift(0.0)
    if K.cmp("I-Imax", I - Imax, ">="):
        Ipen = -muI*(I - Imax)
    d = [None] * 8
    d[0] = -Rt / Tinf / N*S*I
    d[1] = Rt / Tinf / N*S*I - E / Tinc
    d[2] = E / Tinc - I / Tinf
    d[3] = I / Tinf
    d[4] = (pS - pE)*R*I / Tinf / N
    d[5] = (pE - pI) / Tinc
    d[6] = (pS - pE)*R*S / Tinf / N + (pI - pR) / Tinf + Ipen
    d[7] = K.lift(0.0)
    return d, [u], None


def covid_fast(K, P, sw, t, X):
    """The throughput flavour's structure (models_fast.hpp: CovidFast::rhs).  Returns Xdot[8]."""
    Sx, E, I, R, pS, pE, pI, pR = X
    R0, Tinf, Tinc, N, Imax, muI, umin, umax = P
    iTinf, iTinc, iN = K.rcp(Tinf), K.rcp(Tinc), K.rcp(N)
    k = iTinf * iN
    u = (pE - pS) * Sx * I * k * R0
    if K.cmp("u-umin", u - umin, "<"):
        u = umin
    if K.cmp("u-umax", u - umax, ">"):
        u = umax
    Rt = R0 * (1 - u)
    dI = I - Imax
    Ipen = -muI * dI if K.cmp("I-Imax", dI, ">=") else K.lift(0.0)
    flux = Rt * k * Sx * I
    EoT, IoT = E * iTinc, I * iTinf
    dp = (pS - pE) * R * k
    d = [None] * 8
    d[0] = -flux
    d[1] = flux - EoT
    d[2] = EoT - IoT
    d[3] = IoT
    d[4] = dp * I
    d[5] = (pE - pI) * iTinc
    d[6] = dp * Sx + (pI - pR) * iTinf + Ipen
    d[7] = K.lift(0.0)
    return d


MODELS = {"goddard": (goddard_ref, goddard_fast), "covid": (covid_ref, covid_fast)}


def run(fn, K, P, sw, t, X):
    """fn on the kit's numbers; rows arrive as doubles."""
    L = K.lift
    with np.errstate(all="ignore"):
        return fn(K, [L(p) for p in P], [L(s) for s in sw], L(t), [L(xv) for xv in X])


def emulate_fast(model, P, sw, t, X, **mutation):
    """The fast structure in numpy.float64 (one rounding per operation): Xdot as an array."""
    return np.array(run(MODELS[model][1], F64Kit(**mutation), P, sw, t, X), dtype=F64)


# ---- the instrument: value, B_ref, B_fast, decidability ---------------------------------------------------------------------

def _up(e):
    """mpf bound -> double, rounded up."""
    f = float(e)
    return f if mpf(f) >= e else float(np.nextafter(f, np.inf))


def _pin(tracked):
    """[Tracked] -> (value rounded once to double, bound of |computed - that double|): the bound carries the distance between
    the exact value and its double, which a correctly rounded result may be away from the stored double."""
    val = np.array([float(q.v) for q in tracked], dtype=F64)
    bnd = np.array([_up(q.e + abs(q.v - mpf(float(q.v)))) for q in tracked], dtype=F64)
    return val, bnd


def evaluate_row(model, P, sw, t, X, flip=()):
    """One row through both restatements on Tracked numbers.  Returns a dict: value[s], B_ref[s], B_fast[s], decidable,
    undecided (names), margins {name: (value, err_ref, err_fast)} and, for Goddard, u[3], B_u[3], H, B_H (reference order: the
    throughput flavour evaluates control and Hamiltonian by the reference-order code under contraction)."""
    ref, fast = MODELS[model]
    Kr, Kf = TrackedKit(flip), TrackedKit(flip)
    d_ref, u_ref, H_ref = run(ref, Kr, P, sw, t, X)
    d_fast = run(fast, Kf, P, sw, t, X)
    out = {}
    out["value"], out["B_ref"] = _pin(d_ref)
    out["B_fast"] = _pin(d_fast)[1]
    # the two restatements are the same function: their 240-bit values agree far below a double's spacing
    assert all(abs(a.v - b.v) <= mpf(2) ** -150 * (abs(a.v) + abs(b.v)) + mpf(2) ** -1200 for a, b in zip(d_ref, d_fast)), \
        "the two restatements disagree"
    out["undecided"] = sorted(set(Kr.undecided()) | set(Kf.undecided()))
    out["decidable"] = not out["undecided"]
    out["margins"] = {n: (float(m.v), float(m.e), float(Kf.margins[n].e) if n in Kf.margins else float("nan"))
                      for n, m in Kr.margins.items()}
    out["u"], out["B_u"] = _pin(u_ref)
    if H_ref is not None:
        h, bh = _pin([H_ref])
        out["H"], out["B_H"] = h[0], bh[0]
    return out


def value_mpf(model, P, sw, t, X):
    """The mathematical right-hand side in mpf, X given as mpf (the RK4 reference runs on this)."""
    K = MpfKit()
    L = K.lift
    return MODELS[model][0](K, [L(p) for p in P], [L(s) for s in sw], t, list(X))[0]


def rk4_mpf(model, P, sw, t0, X0, step, nsteps):
    """nsteps classical RK4 steps of size `step` (a double) in mpf: X + (h/6) (F1 + (F4 + 2 (F2 + F3)))."""
    h = mpf(float(step))
    t = mpf(float(t0))
    X = [mpf(float(q)) for q in X0]
    f = lambda tt, Y: value_mpf(model, P, sw, tt, Y)
    for _ in range(nsteps):
        F1 = f(t, X)
        F2 = f(t + h / 2, [a + h / 2 * k for a, k in zip(X, F1)])
        F3 = f(t + h / 2, [a + h / 2 * k for a, k in zip(X, F2)])
        F4 = f(t + h, [a + h * k for a, k in zip(X, F3)])
        X = [a + h / 6 * (k1 + (k4 + 2 * (k2 + k3))) for a, k1, k2, k3, k4 in zip(X, F1, F2, F3, F4)]
        t = t + h
    return X
