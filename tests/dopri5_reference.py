"""The adaptive Dormand-Prince 5(4) integrator replayed step by step over the number kits of fast_reference.py (helper of
test_dopri5_pin_cpu.py, test_gpu_dopri5_pin.py and golden/make_dopri5_golden.py, not a test).

TABLEAU.  Typed from the published table (Dormand & Prince, "A family of embedded Runge-Kutta formulae", J. Comput. Appl. Math. 6
(1980), the RK5(4)7M pair; the same table is Hairer, Norsett & Wanner, Solving ODEs I, Table II.5.2) as exact rationals: NODES,
STAGES, B5 (fifth order, the solution that is propagated) and B4 (fourth order, the embedded one).  test_dopri5_pin_cpu.py checks
the order conditions in rational arithmetic and the table against SciPy's own copy.

REPLAY.  `replay` restates Lane::dopri5_try / integrate_dopri5 (socp_amd/csrc/integrator.hpp) -- and with them the copy in
traj_var_wave_dopri5_kernel (variational.hpp) and dopri5_try_step / integrate_dopri5_any (oracle/socp_oracle.c) -- statement for
statement over a kit: stage sums left to right, 1.0 * x + (h * b) * k ...; every coefficient FORMED IN THE KIT as the quotient (or
the difference of two quotients, for the error weights) the kernel forms in double, so that its rounding is inside the bound; the
error norm max_i |e_i| / (tol + tol (|x_i| + h |k1_i|)) on the OLD state; the controller; the double loop with its two eps
comparisons and the re-initialisation h = tf - t.  The same text runs on
    D5Tracked    value (240 bit) and first-order running error bound -- the fixture,
    D5Mpf        value alone,
    D5F64        numpy.float64, one rounding per operation -- the CPU emulation and the carrier of the mutation checks.

ERROR MODEL.  That of fast_reference.Tracked (one rounding u |res| per operation, first-order propagation), plus
    pow(a, p)    |p| |res| ea / |a| + C_POW u |res|, C_POW = 16: OpenCL's limit for double pow.  The device library's real figure is
                 not known to us; `c_pow` of the kit is a parameter so that its share of a bound can be reported.
    max_i        where one component of the error norm wins by more than the bounds of both, that component; otherwise value
                 max_i v_i with bound max_i e_i (|max a - max b| <= max |a_i - b_i|): no decision is needed for the norm.
A fused multiply-add (the throughput flavour's translation unit is compiled with contraction) is a product and a sum, two
roundings: an upper bound.

SOURCES.  A plain running error analysis knows no cancellation, and this loop lives on it: the error estimate is a sum
h (dc1 k1 + dc3 k3 + ...) that cancels to ~tol |x| / (h |k|) of its terms, so an error dh of the step size -- the SAME dh in every
term -- would be charged that factor (10^3 .. 10^5) and again at every later step: bounds that grow 10^4-fold per accepted step
and leave nothing decidable after two.  The numbers of the bound (Affine) therefore carry, beside the local bound e, the
derivative d_j of their value with respect to named SOURCES: at the end of every trial step the accumulated bound of the new
step size, of the new time and of every component of the accepted state is promoted to a source (bound beta_j, derivative 1),
and from there on everything computed from it carries its exact first-order dependence on that one unknown.  What cancels in the
computation then cancels in the bound: |computed - v| <= e + sum_j |d_j| beta_j.  In particular t + h - tf with h = tf - t is
bounded by u (|h| + |tf|) whatever the error of t, as it is on the device.  The derivative rows are float64 (AD_SLACK covers their
own rounding).  Roundings inside one trial step are still summed without cancellation, which is what leaves the observed
error / bound ratios near 0.3 rather than near 1.

DECISIONS.  Every comparison goes through the kit's cmp and is recorded with its margin, in order: err <= 1, f > 0.2, err < 0.5,
err > 5^-5, the two loop conditions, and every kink of the right-hand side at every stage.  A scenario is DECIDABLE when every
margin exceeds DECIDE_FACTOR x its bound.  The loop conditions at the end of a segment have margin eps = 2u against a bound of
u (|h| + |tf|): decidable iff |h| + |tf| < 1/2, so the scenarios keep tf <= 1/4.

MODELS WITH A HOOK OR A MAP.  `replay` also takes a start time other than zero, a right-hand side with auxiliary scalars and a hook
called before every step (the interceptor's chart change), and D5Tracked has every function the interceptor and vtolUAV call -- sin,
cos, tan, acos, atan2, tanh, the library exp, the short sincos, copysign -- each with its derivative row and the budget the model's
own module uses (fast_reference.C_*, interceptor_reference.C_SINCOS_FAST).  adaptive_models_reference.py composes them.
"""
from fractions import Fraction as Fr

import numpy as np

import fast_reference as fr
from fast_reference import F64, DECIDE_FACTOR, HAVE_MPMATH, mpf, mpmath

C_POW = 16
EPS = 2.220446049250313e-16
MAX_TRIALS = 40                    # a replayed scenario is short: the replay stops there and says so ("truncated")

# ---- the Dormand-Prince 5(4) pair, from the literature ---------------------------------------------------------------------
NODES = [Fr(0), Fr(1, 5), Fr(3, 10), Fr(4, 5), Fr(8, 9), Fr(1), Fr(1)]
STAGES = [
    [],
    [Fr(1, 5)],
    [Fr(3, 40), Fr(9, 40)],
    [Fr(44, 45), Fr(-56, 15), Fr(32, 9)],
    [Fr(19372, 6561), Fr(-25360, 2187), Fr(64448, 6561), Fr(-212, 729)],
    [Fr(9017, 3168), Fr(-355, 33), Fr(46732, 5247), Fr(49, 176), Fr(-5103, 18656)],
    [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84)],
]
B5 = [Fr(35, 384), Fr(0), Fr(500, 1113), Fr(125, 192), Fr(-2187, 6784), Fr(11, 84), Fr(0)]
B4 = [Fr(5179, 57600), Fr(0), Fr(7571, 16695), Fr(393, 640), Fr(-92097, 339200), Fr(187, 2100), Fr(1, 40)]

MUTATIONS = {
    "dc7_sign": "the last error weight with the opposite sign",
    "b54_rel": "one stage coefficient (b54) off by 1e-9 relative",
    "norm_on_new": "the error norm taken on the new state",
    "no_hk1": "the error norm without h |k1|",
    "safety_08": "safety factor 0.8 instead of 0.9",
    "no_floor": "no 5^-5 floor under err in the growth formula",
    "no_clamp": "no 0.2 clamp on the shrink factor",
    "threshold_04": "growth threshold 0.4 instead of 0.5",
    "reject_exp_4": "exponent -1/4 instead of -1/3 on rejection",
}


# ---- kits: fast_reference's, with pow, a maximum, and decisions recorded in order under a running prefix --------------------

class _Trail:
    prefix = ""

    def cmp(self, name, m, op):
        name = self.prefix + name
        d = super().cmp(name, m, op)
        self.taken[name] = d
        return d

    def cmp_exact(self, name, a, b, op):
        return super().cmp_exact(self.prefix + name, a, b, op)

    def start(self, nsrc=0):
        self.taken = {}
        self.margins = {}
        return self


class D5Mpf(_Trail, fr.MpfKit):
    def pow(self, a, p):
        return mpmath.power(a, mpf(p))

    def vmax(self, xs):
        return max(xs)

    def promote(self, x):
        return x


class Affine:
    """value v (mpf), local first-order bound e (mpf) of the roundings since the last promotion, and d (float64 array or None = 0):
    the derivative of the value with respect to every SOURCE -- an error that was promoted to a named unknown of known bound, see
    the module docstring.  The bound of |computed - v| is e + sum_j |d_j| beta_j (D5Tracked.total)."""
    __slots__ = ("v", "e", "d")

    def __init__(self, v, e=0, d=None):
        self.v = v if isinstance(v, mpf) else mpf(float(v))
        self.e = e if isinstance(e, mpf) else mpf(e)
        self.d = d

    @staticmethod
    def lift(x):
        return x if isinstance(x, Affine) else Affine(x)

    @property
    def exact(self):
        """No bound at all: an input, or a structural zero (interceptor_reference.lu6_solve leaves those out)."""
        return self.e == 0 and (self.d is None or not self.d.any())

    @staticmethod
    def _rounded(res, prop, d, c=1, underflow=True):
        a = abs(res)
        e = prop + c * fr.U * a
        if underflow and 0 < a < fr.TINY:
            e += fr.ETA
        return Affine(res, e, d)

    @staticmethod
    def _lin(ca, da, cb, db):
        """ca * da + cb * db on derivative rows that may be None."""
        if da is None and db is None:
            return None
        if db is None:
            return float(ca) * da
        if da is None:
            return float(cb) * db
        return float(ca) * da + float(cb) * db

    def __neg__(self):
        return Affine(-self.v, self.e, None if self.d is None else -self.d)

    def __abs__(self):
        return -self if self.v < 0 else self

    def __add__(self, o):
        o = Affine.lift(o)
        return Affine._rounded(self.v + o.v, self.e + o.e, Affine._lin(1, self.d, 1, o.d), underflow=False)

    __radd__ = __add__

    def __sub__(self, o):
        o = Affine.lift(o)
        return Affine._rounded(self.v - o.v, self.e + o.e, Affine._lin(1, self.d, -1, o.d), underflow=False)

    def __rsub__(self, o):
        return Affine.lift(o) - self

    def __mul__(self, o):
        o = Affine.lift(o)
        prop = abs(self.v) * o.e + abs(o.v) * self.e
        if fr.Tracked.second_order:                     # fast_reference.second_order_products(): vtolUAV's vanishing factors
            prop += self.e * o.e
        return Affine._rounded(self.v * o.v, prop, Affine._lin(o.v, self.d, self.v, o.d))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Affine.lift(o)
        res = self.v / o.v
        return Affine._rounded(res, (self.e + abs(res) * o.e) / abs(o.v), Affine._lin(1 / o.v, self.d, -res / o.v, o.d))

    def __rtruediv__(self, o):
        return Affine.lift(o) / self


class D5Tracked(_Trail, fr._Kit):
    """The bound.  fast_reference.TrackedKit's error model on Affine numbers, with pow and the maximum of the error norm."""
    AD_SLACK = 1 + 2.0 ** -20                            # the derivative rows are float64: their own rounding, generously

    def __init__(self, flip=(), c_pow=C_POW, c_exp=fr.C_EXP):
        super().__init__(flip)
        self.c_pow = c_pow
        self.c_exp = c_exp                              # vtolUAV's throughput flavour calls the library's exp: C_EXP_LIB

    def start(self, nsrc=0):
        super().start()
        self.beta = np.zeros(nsrc)
        self.nsrc = 0
        return self

    def lift(self, x):
        return Affine(x)

    def value(self, x):
        return x.v

    def total(self, x):
        """Bound of |computed - x.v|."""
        if x.d is None:
            return x.e
        return x.e + mpf(float(np.dot(np.abs(x.d), self.beta)) * self.AD_SLACK)

    def promote(self, x):
        """The local bound of x becomes a source: from here on everything computed from x carries its exact first-order
        dependence on that one unknown, so that what cancels in the computation cancels in the bound."""
        if x.e == 0:
            return x
        d = np.zeros(len(self.beta)) if x.d is None else x.d.copy()
        d[self.nsrc] = 1.0
        self.beta[self.nsrc] = fr._up(x.e)
        self.nsrc += 1
        return Affine(x.v, 0, d)

    @staticmethod
    def sqrt(a):
        res = mpmath.sqrt(a.v)
        if res == 0:                                    # the root of an exact zero (thrust off): nothing to propagate
            assert a.e == 0 and (a.d is None or not a.d.any())
            return Affine(res)
        return Affine._rounded(res, a.e / (2 * res) if a.e else mpf(0), Affine._lin(1 / (2 * res), a.d, 0, None))

    def exp(self, a, c=None):
        res = mpmath.exp(a.v)
        e = res * a.e + (self.c_exp if c is None else c) * fr.U * res
        if res < fr.TINY:
            e += fr.EXP_FLOOR
        return Affine(res, e, Affine._lin(res, a.d, 0, None))

    def exp_lib(self, a):
        """The device library's exp as the interceptor's throughput flavour calls it (interceptor_reference.FastTrackedKit)."""
        return self.exp(a, fr.C_EXP_LIB)

    # The functions the interceptor and vtolUAV call, each with its derivative row and the budget its model module uses
    # (fast_reference.TrackedKit's error model, term for term).
    @staticmethod
    def _fn(res, prop, c, da, d):
        return Affine(res, prop + c * fr.U * abs(res), Affine._lin(da, d, 0, None))

    @staticmethod
    def tanh(a):
        res = mpmath.tanh(a.v)
        return D5Tracked._fn(res, (1 - res * res) * a.e, fr.C_TANH, 1 - res * res, a.d)

    @staticmethod
    def sin(a):
        res, c = mpmath.sin(a.v), mpmath.cos(a.v)
        return D5Tracked._fn(res, abs(c) * a.e, fr.C_SIN, c, a.d)

    @staticmethod
    def cos(a):
        res, s = mpmath.cos(a.v), mpmath.sin(a.v)
        return D5Tracked._fn(res, abs(s) * a.e, fr.C_COS, -s, a.d)

    @staticmethod
    def tan(a):
        res = mpmath.tan(a.v)
        return D5Tracked._fn(res, (1 + res * res) * a.e, fr.C_TAN, 1 + res * res, a.d)

    @staticmethod
    def atan2(y, x, y_negative_zero=False):
        res = fr._atan2_mpf(y.v, x.v, y_negative_zero)
        n2 = x.v * x.v + y.v * y.v
        if not n2:
            return Affine(res, fr.C_ATAN2 * fr.U * abs(res))
        return Affine(res, (abs(x.v) * y.e + abs(y.v) * x.e) / n2 + fr.C_ATAN2 * fr.U * abs(res), Affine._lin(x.v / n2, y.d, -y.v / n2, x.d))

    @staticmethod
    def acos(a):
        """The enclosure of TrackedKit.acos for the local bound; the sources enter to first order, -1 / sqrt(1 - a^2)."""
        v = fr._clamp1(a.v)
        res = mpmath.acos(v)
        prop = max(mpmath.acos(fr._clamp1(v - a.e)) - res, res - mpmath.acos(fr._clamp1(v + a.e))) if a.e else mpf(0)
        d = None
        if a.d is not None and a.d.any():
            assert abs(v) < 1, "acos at +-1 of a number that depends on a source: no first-order bound"
            d = float(-1 / mpmath.sqrt(1 - v * v)) * a.d
        return Affine(res, prop + fr.C_ACOS * fr.U * abs(res), d)

    @staticmethod
    def copysign(a, b):
        pos = b.v >= 0
        same = (a.v >= 0) == pos
        return Affine(abs(a.v) if pos else -abs(a.v), a.e, a.d if same or a.d is None else -a.d)

    @staticmethod
    def sincos_fast(a, c_rel, k_abs):
        """ifast::sincos (interceptor_reference._sincos_fast): relative budget c_rel u and the absolute part k_abs of the reduction."""
        s, c = mpmath.sin(a.v), mpmath.cos(a.v)
        return (Affine(s, abs(c) * (a.e + k_abs) + c_rel * fr.U * abs(s), Affine._lin(c, a.d, 0, None)),
                Affine(c, abs(s) * (a.e + k_abs) + c_rel * fr.U * abs(c), Affine._lin(-s, a.d, 0, None)))

    def exact_diff(self, a, b):
        """fast_reference's cmp_exact compares two INPUTS; along a trajectory the position is computed, so the difference carries
        its operands' bounds (and no rounding of its own: only its sign is read) and the decision is judged like any other."""
        return Affine(a.v - b.v, a.e + b.e, Affine._lin(1, a.d, -1, b.d))

    @staticmethod
    def rcp(a):
        res = 1 / a.v
        return Affine._rounded(res, a.e * res * res, Affine._lin(-res * res, a.d, 0, None), c=fr.C_RCP)

    @staticmethod
    def rsqrt(a):
        res = 1 / mpmath.sqrt(a.v)
        return Affine._rounded(res, a.e * abs(res) / (2 * abs(a.v)) if a.e else mpf(0), Affine._lin(-res / (2 * a.v), a.d, 0, None),
                               c=fr.C_RSQ)

    def pow(self, a, p):
        p = mpf(p)
        res = mpmath.power(a.v, p)
        return Affine(res, abs(p) * res * a.e / abs(a.v) + self.c_pow * fr.U * res, Affine._lin(p * res / a.v, a.d, 0, None))

    def vmax(self, xs):
        """The maximum of the error norm.  Where one component wins by more than the bounds of both, the computed maximum is that
        component's computed value and the result keeps its derivative row; otherwise |max a - max b| <= max |a_i - b_i|."""
        tot = [self.total(x) for x in xs]
        w = max(range(len(xs)), key=lambda i: xs[i].v)
        if all(i == w or xs[w].v - xs[i].v > tot[w] + tot[i] for i in range(len(xs))):
            return xs[w]
        return Affine(xs[w].v, max(tot))

    def decidable(self):
        return not self.undecided()

    def undecided(self):
        out = []
        for n, m in self.margins.items():
            t = self.total(m)
            if not (t == 0 or abs(m.v) > DECIDE_FACTOR * t):
                out.append(n)
        return out


class D5F64(_Trail, fr.F64Kit):
    def pow(self, a, p):
        return np.power(a, F64(p))

    def vmax(self, xs):
        err = F64(0.0)
        for e in xs:                                    # the kernel's loop: if (e > err || e != e) err = e
            if e > err or e != e:
                err = e
        return err

    def promote(self, x):
        return x


# ---- right-hand sides ------------------------------------------------------------------------------------------------------
# double integrator, parameter block u_max, a_max, muT (socp_amd/csrc/models_exact.hpp: DIntExact; models_variational.hpp: DIntVar)

def dint_control(K, P, X):
    """DIntExact::control_only: u = -p_v / a_max, rescaled to u_max when its norm exceeds it (the saturation kink)."""
    u_max, a_max = P[0], P[1]
    u = [-X[9] / a_max, -X[10] / a_max, -X[11] / a_max]
    norm_u = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    if K.cmp("norm_u-u_max", norm_u - u_max, ">"):
        u = [ui / norm_u*u_max for ui in u]
    return u


def dint_rhs(K, P, sw, t, X):
    """DIntExact::rhs.  Returns Xdot[12]."""
    u = dint_control(K, P, X)
    a_max = P[1]
    zero = K.lift(0.0)
    return [X[3], X[4], X[5], a_max * u[0], a_max * u[1], a_max * u[2], zero, zero, zero, -X[6], -X[7], -X[8]]


def dint_aug_rhs(K, P, sw, t, Y):
    """DIntVar::aug_rhs for e = 0 .. 155, in its operation order.  The kernel writes the sensitivity rows as 0.0 + (+-1.0) * Y[.]:
    both operations are exact in IEEE arithmetic, so they are written here as the (negated) element and count no rounding."""
    S = 12
    d = dint_rhs(K, P, sw, t, Y[:S])
    zero = K.lift(0.0)
    for i in range(S):
        for j in range(S):
            if i < 3:
                d.append(Y[S + S * (i + 3) + j])
            elif i < 6:
                d.append(-Y[S + S * (i + 6) + j])
            elif i < 9:
                d.append(zero)
            else:
                d.append(-Y[S + S * (i - 3) + j])
    return d


RHS = {
    ("goddard", "ref"): lambda K, P, sw, t, X: fr.goddard_ref(K, P, sw, t, X)[0],
    ("goddard", "fast"): fr.goddard_fast,
    ("covid", "ref"): lambda K, P, sw, t, X: fr.covid_ref(K, P, sw, t, X)[0],
    ("covid", "fast"): fr.covid_fast,
    ("dint", "ref"): dint_rhs,
    ("dint_aug", "ref"): dint_aug_rhs,
}
FLAVOURS = {"goddard": ("ref", "fast"), "covid": ("ref", "fast"), "dint": ("ref",), "dint_aug": ("ref",)}
KINKS = ("Switch", "Switch+2mu2umax", "t-sw0", "t-sw1", "|alpha|-umax", "u-umin", "u-umax", "I-Imax", "norm_u-u_max")


# ---- the replay ------------------------------------------------------------------------------------------------------------

HOOK_MUTATIONS = {
    "stale_k1": "the FSAL derivative kept after the hook rewrote the state",
}


def replay(K, model, flavour, P, sw, tol, tf, step_nbr, X0, mut=None, t0=0.0, rhs=None, aux=None, hook=None, resume=None,
           h0_from=None, max_trials=MAX_TRIALS):
    """integrate_dopri5(t0, tf) on the kit K.  Returns a dict: times / states (t0 and the end of every accepted step, kit
    numbers), trials [dict(step, t, h, err, accepted, fresh, clamp, start_taken: the kink decisions at the step's
    start)], stage_taken (the decisions of the stages of each trial).  `mut` names one entry of MUTATIONS or HOOK_MUTATIONS.

    t0 != 0: h0 = (tf - t0) / step_nbr has a rounded subtraction, which is counted (and promoted to a source, as every later step
    size is).  rhs(K, t, X, aux) replaces the table's right-hand side (model, flavour, P and sw are then unused); aux is whatever
    the model carries beside the state (the interceptor's stage and chart, vtolUAV's lifted obstacle table).  hook(K, t, X, aux) ->
    (changed, X, aux) is called where integrate_dopri5 calls its hook: before every step, inside the inner loop; its decisions go
    through K.cmp under the prefix H<n>.; when it reports a change k1 is recomputed at the new X.  The result has `aux` (one entry
    per row of states) and `hooks` (per call: whether it changed the state, and the index of the trial that follows).  resume: the
    result of the segment run just before this one on the SAME kit -- the kit is not restarted, X0 are its numbers, and rows,
    trials and decision names count on (the interceptor's second phase).  h0_from: the first step formed from tf - h0_from (a
    mutation of the callers').  max_trials: where the replay stops and says "truncated"; it also sizes the sources."""
    assert mut is None or mut in MUTATIONS or mut in HOOK_MUTATIONS, mut
    L = K.lift
    if resume is None:
        K.start((len(X0) + 2) * (max_trials + 2))
    if rhs is None:
        table_rhs = RHS[(model, flavour)]
        Pk, swk = [L(p) for p in P], [L(s) for s in sw]
        rhs = lambda K_, t_, X_, aux_: table_rhs(K_, Pk, swk, t_, X_)
    n = len(X0)

    def q(c):                                           # a coefficient as the kernel forms it: numerator / denominator in double
        return L(c.numerator) / L(c.denominator)

    a = [q(c) for c in NODES]
    b = [[q(c) for c in row] for row in STAGES]
    if mut == "b54_rel":
        b[4][3] = b[4][3] * L(1.0 + 1e-9)
    c5 = [q(c) for c in B5]
    dc = [q(c5_) - q(c4_) for c5_, c4_ in zip(B5[:6], B4[:6])] + [q(-B4[6])]
    if mut == "dc7_sign":
        dc[6] = -dc[6]
    one, half, c02 = L(1.0), L(0.4 if mut == "threshold_04" else 0.5), L(0.2)
    c09 = L(0.8 if mut == "safety_08" else 0.9)
    p_rej = -1.0 / 4.0 if mut == "reject_exp_4" else -1.0 / 3.0
    floor5 = one / L(3125.0)
    eps, tolk, tfk = L(EPS), L(tol), L(tf)

    def f(tag, t, X):
        K.prefix = tag
        out = rhs(K, t, X, aux)
        K.prefix = ""
        return out

    def sums(X, hh, coef, ks):                          # 1.0 * x + h * c1 * k1 + h * c2 * k2 ..., left to right, zero weights left out
        hc = [(hh * c, k) for c, k in zip(coef, ks) if k is not None]
        out = []
        for i in range(n):
            s = X[i]
            for w, k in hc:
                s = s + w * k[i]
            out.append(s)
        return out

    t = L(float(t0))
    # h0 = (tf - t0) / step_nbr with t0 = 0: the subtraction is exact, and so is the division when step_nbr is 1
    if t0 == 0.0 and h0_from is None:
        h = tfk if step_nbr == 1 else tfk / L(float(step_nbr))
    else:
        h = tfk - L(float(t0 if h0_from is None else h0_from))
        h = K.promote(h if step_nbr == 1 else h / L(float(step_nbr)))
    if resume is None:
        X = [L(x) for x in X0]
        res = {"times": [t], "states": [X], "aux": [aux], "trials": [], "stage_taken": [], "hooks": [], "outer": 0, "step": 0}
    else:
        X = list(X0)
        res = {k: (list(v) if isinstance(v, list) else v) for k, v in resume.items()}
        res["times"].append(t)
        res["states"].append(X)
        res["aux"].append(aux)
    if not K.value(h) > 0:
        return res
    k1 = None
    fresh = False                                       # h is tf - t, formed at this t and not resized since
    step = res["step"]
    outer = res["outer"]
    while K.cmp("O%d.tf-t>eps" % outer, (tfk - t) - eps, ">"):
        while True:
            if not K.cmp("I%d.t+h-tf<=eps" % len(res["trials"]), (t + h - tfk) - eps, "<="):
                break
            if hook is not None:
                K.prefix = "H%d." % len(res["hooks"])
                changed, X, aux = hook(K, t, X, aux)
                K.prefix = ""
                res["hooks"].append((bool(changed), len(res["trials"])))
                if changed and mut != "stale_k1":
                    k1 = None
            if k1 is None:
                k1 = f("S%d.k1." % step, t, X)
                start_taken = {k.split(".", 2)[2]: v for k, v in K.taken.items() if k.startswith("S%d.k1." % step)}
            while True:
                T = len(res["trials"])
                if T >= max_trials:                     # (a mutated controller may not get there: its rows so far are kept)
                    res["truncated"] = True
                    return res
                tag = "T%d." % T
                hh, tt = h, t
                k2 = f(tag + "k2.", tt + hh * a[1], sums(X, hh, b[1], [k1]))
                k3 = f(tag + "k3.", tt + hh * a[2], sums(X, hh, b[2], [k1, k2]))
                k4 = f(tag + "k4.", tt + hh * a[3], sums(X, hh, b[3], [k1, k2, k3]))
                k5 = f(tag + "k5.", tt + hh * a[4], sums(X, hh, b[4], [k1, k2, k3, k4]))
                k6 = f(tag + "k6.", tt + hh, sums(X, hh, b[5], [k1, k2, k3, k4, k5]))
                xn = sums(X, hh, c5[:6], [k1, None, k3, k4, k5, k6])
                kn = f(tag + "k7.", tt + hh, xn)
                es = []
                for i in range(n):
                    e = (hh * dc[0]) * k1[i]
                    for w, k in ((dc[2], k3), (dc[3], k4), (dc[4], k5), (dc[5], k6), (dc[6], kn)):
                        e = e + (hh * w) * k[i]
                    x_i = abs(xn[i]) if mut == "norm_on_new" else abs(X[i])
                    den = tolk + tolk * (x_i if mut == "no_hk1" else x_i + hh * abs(k1[i]))
                    es.append(abs(e) / den)
                err = K.vmax(es)
                trial = {"step": step, "t": tt, "h": hh, "err": err, "fresh": fresh, "clamp": False, "start_taken": start_taken}
                res["trials"].append(trial)
                res["stage_taken"].append({k: v for k, v in K.taken.items() if k.startswith(tag)})
                ok = K.cmp(tag + "err<=1", err - one, "<=")
                trial["accepted"] = ok
                if not ok:
                    fac = c09 * K.pow(err, p_rej)
                    if mut != "no_clamp" and not K.cmp(tag + "f>0.2", fac - c02, ">"):
                        fac = c02
                        trial["clamp"] = True
                    h = K.promote(hh * fac)
                    fresh = False
                    continue
                t = K.promote(tt + hh)
                if K.cmp(tag + "err<0.5", err - half, "<"):
                    e = err
                    if mut != "no_floor" and not K.cmp(tag + "err>5^-5", err - floor5, ">"):
                        e = floor5
                    h = K.promote(hh * (c09 * K.pow(e, -1.0 / 5.0)))
                    fresh = False
                break
            X, k1 = [K.promote(x) for x in xn], kn      # FSAL: the next step starts from the accepted trial's last stage
            start_taken = {k.split(".", 2)[2]: v for k, v in res["stage_taken"][-1].items() if k.startswith(tag + "k7.")}
            step += 1
            res["step"] = step
            res["times"].append(t)
            res["states"].append(X)
            res["aux"].append(aux)
        h = tfk - t
        fresh = True
        k1 = None
        outer += 1
        res["outer"] = outer
    return res


def emulate(model, flavour, P, sw, tol, tf, step_nbr, X0, mut=None):
    """The replay in numpy.float64: (times[rows], states[rows][n], accepted, rejected)."""
    with np.errstate(all="ignore"):
        r = replay(D5F64(), model, flavour, P, sw, tol, tf, step_nbr, X0, mut)
    acc = sum(1 for tr in r["trials"] if tr["accepted"])
    return (np.array(r["times"], dtype=F64), np.array(r["states"], dtype=F64), acc, len(r["trials"]) - acc)


# ---- the instrument --------------------------------------------------------------------------------------------------------

def branches(r, step_nbr, value=float, kinks=KINKS):
    """The rows of the controller's branch table a replay went through (names of BRANCHES).  kinks: the decision names that count
    as a kink of the right-hand side, or a predicate on the name."""
    is_kink = kinks if callable(kinks) else (lambda name: name in kinks)
    out = set()
    tr = r["trials"]
    v = [value(x["err"]) for x in tr]
    for i, x in enumerate(tr):
        if x["accepted"]:
            if v[i] < 5.0 ** -5:
                out.add("cap")
                if step_nbr == 1 and len(tr) == 1:
                    out.add("single_cap")
            elif v[i] < 0.5:
                # the next trial is taken at the grown size (not at a re-initialised one)
                if i + 1 < len(tr) and not tr[i + 1]["fresh"]:
                    out.add("grow")
                    if v[i] >= 0.4:                     # ... and a growth threshold of 0.4 would have kept the size
                        out.add("grow_04")
            else:
                out.add("keep")
        else:
            out.add("clamp" if x["clamp"] else "reject")
            if i + 1 < len(tr) and not tr[i + 1]["accepted"]:
                out.add("reject2")
            if x["fresh"]:
                out.add("reinit_reject")
        if x["fresh"] and x["step"] > 0:
            out.add("reinit")
    # a stage on the other side of a control kink than the step's start
    for x, st in zip(tr, r["stage_taken"]):
        start = x["start_taken"]
        for k, d in st.items():
            name = k.split(".", 2)[2]
            if is_kink(name) and name in start and start[name] != d:
                out.add("kink")
    return out


BRANCHES = ["single_cap", "cap", "grow", "grow_04", "keep", "reject", "clamp", "reject2", "reinit", "reinit_reject", "kink"]


def _pin(K, xs):
    """[Affine] -> (value rounded once to double, bound of |computed - that double|), as fast_reference._pin."""
    val = np.array([float(q.v) for q in xs], dtype=F64)
    bnd = np.array([fr._up(K.total(q) + abs(q.v - mpf(float(q.v)))) for q in xs], dtype=F64)
    return val, bnd


def evaluate_scenario(sc, c_pow=C_POW):
    """One scenario (dict: model, P, sw, tol, tf, step_nbr, X0) through the Tracked replay of every flavour of its model.  Returns a
    dict: times[rows], Bt_ref / Bt_fast[rows]; states[rows][n], B_ref / B_fast[rows][n] (end state = last row); err[trials], accepted[trials], h[trials];
    n_accepted, n_rejected; decidable, undecided (names); branches; trail (text)."""
    out = {}
    runs = {}
    for fl in FLAVOURS[sc["model"]]:
        K = D5Tracked(c_pow=c_pow)
        runs[fl] = (K, replay(K, sc["model"], fl, sc["P"], sc["sw"], sc["tol"], sc["tf"], sc["step_nbr"], sc["X0"]))
    K, r = runs["ref"]
    assert not any("truncated" in rr for _, rr in runs.values()), "scenario too long"
    out["times"] = _pin(K, r["times"])[0]
    und = set()
    for fl, (Kf, rf) in runs.items():
        assert [x["accepted"] for x in rf["trials"]] == [x["accepted"] for x in r["trials"]]
        vals, bnds = zip(*[_pin(Kf, row) for row in rf["states"]])
        if fl == "ref":
            out["states"] = np.array(vals)
        else:
            # the restatements are the same function: their 240-bit trajectories agree far below a double's spacing
            assert all(abs(p.v - s.v) <= mpf(2) ** -120 * (abs(p.v) + abs(s.v)) + mpf(2) ** -1000
                       for rp, rs in zip(r["states"], rf["states"]) for p, s in zip(rp, rs)), "the two restatements disagree"
        out["B_" + fl] = np.array(bnds)
        out["Bt_" + fl] = _pin(Kf, rf["times"])[1]
        und |= set(Kf.undecided())
    out["undecided"] = sorted(und)
    out["decidable"] = not und
    tr = r["trials"]
    out["err"] = np.array([float(x["err"].v) for x in tr])
    out["err_rel"] = np.array([float(K.total(x["err"]) / x["err"].v) if x["err"].v else 0.0 for x in tr])
    out["h"] = np.array([float(x["h"].v) for x in tr])
    out["accepted"] = np.array([x["accepted"] for x in tr])
    out["n_accepted"] = int(out["accepted"].sum())
    out["n_rejected"] = len(tr) - out["n_accepted"]
    out["branches"] = branches(r, sc["step_nbr"], value=lambda e: float(e.v))
    out["trail"] = trail(out)
    return out


def trail(ev):
    """The decision trail as text: one entry per trial step."""
    return " ".join("%s(h=%.3g err=%.3g)" % ("A" if a else "R", h, e) for a, h, e in zip(ev["accepted"], ev["h"], ev["err"]))
