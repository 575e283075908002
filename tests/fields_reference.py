"""The definition of socp_fields_batch (include/socp_hip.h) restated in Python, one IEEE operation per line (helper of
test_fields_cpu.py and test_gpu_fields_batch.py, not a test).

A `Dual` is (v, d) over a carrier: Python floats (IEEE doubles -- the kernel must reproduce every output bit for bit) or mpmath
numbers (the 240-bit truth of the same recurrence).  The rules are the header's: a plain number -- a parameter, a literal, t, h, a
control or penalty that the law makes a constant -- takes part with its zero derivative terms DROPPED, so the mixed operations below
are not the general ones with d = 0 (the two differ in the sign of a zero).

The right-hand sides are the generic-kit texts: fast_reference.goddard_ref and covid_ref as they stand, dint_ref / osc1d_ref
here.  DualKit and PlainKit sit on fast_reference._Kit and use math.exp / math.sqrt (numpy's exp is NOT libm's).
A kit's lift() returns a PLAIN number: the constants those texts lift (thrust off or full, an inactive penalty) stay plain."""
import math

import numpy as np

from fast_reference import _Kit, MpfKit, goddard_ref, covid_ref, mpf, mpmath, HAVE_MPMATH   # noqa: F401
from jacobi_reference import det_reference

COSTATE, ALL = 0, 1


class Dual:
    __slots__ = ("v", "d")
    SQRT = staticmethod(math.sqrt)
    EXP = staticmethod(math.exp)
    SQRT_ZERO_RULE = True            # False: the corrupted restatement without the s == 0 rule
    PRODUCT_BOTH_TERMS = True        # False: the corrupted product rule with one term dropped

    def __init__(self, v, d):
        self.v = v
        self.d = d

    def _new(self, v, d):
        return type(self)(v, d)

    def __neg__(self):
        return self._new(-self.v, -self.d)

    def __abs__(self):
        return self._new(abs(self.v), -self.d if self.v < 0 else self.d)

    def __add__(self, o):
        if isinstance(o, Dual):
            return self._new(self.v + o.v, self.d + o.d)
        return self._new(self.v + o, self.d)

    def __radd__(self, c):
        return self._new(c + self.v, self.d)

    def __sub__(self, o):
        if isinstance(o, Dual):
            return self._new(self.v - o.v, self.d - o.d)
        return self._new(self.v - o, self.d)

    def __rsub__(self, c):
        return self._new(c - self.v, -self.d)

    def __mul__(self, o):
        if isinstance(o, Dual):
            left = self.d * o.v
            right = self.v * o.d
            return self._new(self.v * o.v, left + right if self.PRODUCT_BOTH_TERMS else left)
        return self._new(self.v * o, self.d * o)

    def __rmul__(self, c):
        return self._new(c * self.v, c * self.d)

    def __truediv__(self, o):
        if isinstance(o, Dual):
            q = self.v / o.v
            m = q * o.d
            return self._new(q, (self.d - m) / o.v)
        return self._new(self.v / o, self.d / o)

    def __rtruediv__(self, c):
        q = c / self.v
        m = q * self.d
        return self._new(q, (-m) / self.v)

    def sqrt(self):
        s = self.SQRT(self.v)
        if s == 0 and self.SQRT_ZERO_RULE:
            return self._new(s, np.zeros_like(self.d) if isinstance(self.d, np.ndarray) else type(s)(0.0))
        if s == 0:                                            # IEEE's d / 0, which Python raises on: 0 / 0 = NaN, else an infinity
            with np.errstate(all="ignore"):
                return self._new(s, np.asarray(self.d, dtype=np.float64) / 0.0)
        return self._new(s, self.d / (s + s))

    def exp(self):
        e = self.EXP(self.v)
        return self._new(e, e * self.d)


class DualNoZeroRule(Dual):
    __slots__ = ()
    SQRT_ZERO_RULE = False


if HAVE_MPMATH:
    class DualMpf(Dual):
        """The same rules on 240-bit numbers: the truth of the discrete recurrence."""
        __slots__ = ()
        SQRT = staticmethod(lambda x: mpmath.sqrt(x))
        EXP = staticmethod(lambda x: mpmath.exp(x))


class DualKit(_Kit):
    """Dual numbers (any Dual class) and plain numbers side by side; decisions read the value part."""

    def lift(self, x):
        return x

    def value(self, x):
        return x.v if isinstance(x, Dual) else x

    @staticmethod
    def sqrt(x):
        return x.sqrt() if isinstance(x, Dual) else math.sqrt(x)

    @staticmethod
    def exp(x):
        return x.exp() if isinstance(x, Dual) else math.exp(x)


class PlainKit(_Kit):
    """Python floats with libm's exp and sqrt: must equal the oracle's right-hand side bit for bit."""

    def lift(self, x):
        return float(x)

    def value(self, x):
        return x

    sqrt = staticmethod(math.sqrt)
    exp = staticmethod(math.exp)


class DualMpfKit(DualKit):
    @staticmethod
    def sqrt(x):
        return x.sqrt() if isinstance(x, Dual) else mpmath.sqrt(x)

    @staticmethod
    def exp(x):
        return x.exp() if isinstance(x, Dual) else mpmath.exp(x)


# ---- right-hand sides over a generic kit (the Goddard and covid19 ones are fast_reference's) ------------------------------------

def dint_ref(K, P, sw, t, X):
    """Reference operation order (oracle/socp_oracle.c: dint_control, dint_f).  P = u_max, a_max, muT.  Returns (Xdot[12], u[3], None)."""
    u_max, a_max = P[0], P[1]
    u = [-X[9] / a_max, -X[10] / a_max, -X[11] / a_max]
    norm_u = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    if K.cmp("|u|-umax", norm_u - u_max, ">"):
        u = [ui / norm_u*u_max for ui in u]
    zero = K.lift(0.0)
    d = [X[3], X[4], X[5], a_max * u[0], a_max * u[1], a_max * u[2], zero, zero, zero, -X[6], -X[7], -X[8]]
    return d, u, None


def osc1d_ref(K, P, sw, t, X):
    """tests/plugin/osc1d_plugin.hip and osc1d_fields_plugin.hip: x' = -p, p' = w x."""
    return [-X[1], P[0] * X[0]], [-X[1]], None


RHS = {"goddard": goddard_ref, "covid": covid_ref, "dint": dint_ref, "osc1d": osc1d_ref}


def rhs_on(fn, K, P, sw, t, X):
    """Xdot of a generic-kit text; parameters, switching times and t arrive as the carrier's plain numbers, X as the kit's numbers."""
    return fn(K, list(P), list(sw), t, list(X))[0]


def plain_rhs(model, P, sw, t, X):
    """The restated right-hand side on Python floats (PlainKit): an array."""
    return np.array(rhs_on(RHS[model], PlainKit(), [float(p) for p in P], [float(s) for s in sw], float(t), [float(x) for x in X]))


def _as_dual(cls, q, zero):
    """A right-hand-side component that is a plain constant has the derivative +0.0."""
    return q if isinstance(q, Dual) else cls(q, zero.copy() if isinstance(zero, np.ndarray) else zero)


def rk4_dual(fn, K, cls, P, sw, t, X, h, zero=0.0):
    """One RK4 step in the association order of odeTools.cpp:89-98 (Lane::rk4, jacobi_reference.rk4_of) on dual numbers; t and h are
    plain."""
    f = lambda tt, Y: [_as_dual(cls, q, zero) for q in rhs_on(fn, K, P, sw, tt, Y)]   # noqa: E731
    h2 = h / 2.0
    th = t + h / 2.0
    F1 = f(t, X)
    Y = [x + h2 * k for x, k in zip(X, F1)]
    F2 = f(th, Y)
    Y = [x + h2 * k for x, k in zip(X, F2)]
    F3 = f(th, Y)
    Y = [x + h * k for x, k in zip(X, F3)]
    Fs = [a + b for a, b in zip(F2, F3)]
    F4 = f(t + h, Y)
    h6 = h / 6.0
    return [x + h6 * (k1 + (k4 + 2.0 * ks)) for x, k1, k4, ks in zip(X, F1, F4, Fs)]


def detect(tq, det, skip):
    """DETECTION of the header on the samples of a slab: (nchange, tconj)."""
    nchange, tconj = 0, float("nan")
    for j in range(1, len(det)):
        if j - 1 < skip:
            continue
        d0, d1, t0 = det[j - 1], det[j], tq[j - 1]
        if d0 == d0 and d1 == d1 and (d0 < 0.0) != (d1 < 0.0):
            if nchange == 0:
                den = d0 - d1
                q = d0 / den
                span = tq[j] - t0
                tconj = t0 + span * q
            nchange += 1
    return nchange, tconj


def fields_segment(model, P, sw, D, t1, t2, X0, N, cols=COSTATE, stride=1, skip=0, cls=Dual, kit=None, swap_sign=True, trajectory=None):
    """One slab: dict(tq, det: one entry per sample; count, nchange, tconj, phi[S][C]).  cls = Dual: the definition in doubles;
    cls = DualMpf (with kit = DualMpfKit()): the same recurrence in 240 bits (no determinants), t1 / t2 / P taken as the doubles they
    are and the step sequence that of the doubles.  trajectory: a list that receives the value part after every step.
    In doubles the C columns travel together: one state whose derivative parts are numpy arrays of C doubles -- the value parts of
    all columns are the same numbers and numpy's elementwise products, sums and quotients are the scalar IEEE operations."""
    fn = RHS[model]
    K = kit if kit is not None else DualKit()
    S = 2 * D
    C = S if cols == ALL else D
    high = HAVE_MPMATH and issubclass(cls, DualMpf)
    num = (lambda x: mpf(float(x))) if high else float
    first = 0 if cols == ALL else D
    if high:
        zero = num(0.0)
        states = [[cls(num(X0[j]), num(1.0) if j == first + c else zero) for j in range(S)] for c in range(C)]
        dpart = lambda r, c: states[c][r].d                                                # noqa: E731
    else:
        zero = np.zeros(C)
        unit = lambda j: np.array([1.0 if j == first + c else 0.0 for c in range(C)])      # noqa: E731
        states = [[cls(num(X0[j]), unit(j)) for j in range(S)]]
        dpart = lambda r, c: float(states[0][r].d[c])                                      # noqa: E731
    Pn, swn = [num(p) for p in P], [num(s) for s in sw]
    out = dict(tq=[], det=[])
    # the step sequence is decided in doubles, as the residual decides it
    t1, t2 = float(t1), float(t2)
    dt = (t2 - t1) / N
    t = t1
    guard = N + 8
    k = 0
    act = t < (t2 - dt / 2) and guard > 0
    guard -= 1 if act else 0
    while act:
        h_step = (t2 - t) if (t + dt > t2) else dt
        with np.errstate(all="ignore"):
            states = [rk4_dual(fn, K, cls, Pn, swn, num(t), X, num(h_step), zero) for X in states]
        if trajectory is not None:
            trajectory.append([q.v for q in states[0]])
        tq = t + h_step
        t = t + dt
        k += 1
        act = t < (t2 - dt / 2) and guard > 0
        guard -= 1 if act else 0
        if (k % stride == 0 or not act) and not high:
            J = np.array([[dpart(r, C - D + cc) for cc in range(D)] for r in range(D)])
            out["tq"].append(tq)
            out["det"].append(det_reference(J, swap_sign)[0])
    out["count"] = len(out["det"])
    out["nchange"], out["tconj"] = detect(out["tq"], out["det"], skip)
    out["phi"] = [[dpart(r, c) for c in range(C)] for r in range(S)]
    if not high:
        out["phi"] = np.array(out["phi"], dtype=np.float64)
    return out


def with_skip(slab, skip):
    """The slab another skip gives: only DETECTION reads it."""
    out = dict(slab)
    out["nchange"], out["tconj"] = detect(slab["tq"], slab["det"], skip)
    return out


def costate_columns(slab, D):
    """The cols = COSTATE slab of a cols = ALL one: the columns are independent, the last d are the same numbers."""
    out = dict(slab)
    out["phi"] = np.ascontiguousarray(slab["phi"][:, D:])
    return out


def jend_of(phi, D):
    """The x-rows of the costate columns: J = dx(t_{i+1})/dp(t_i)."""
    C = len(phi[0])
    return [[phi[r][C - D + c] for c in range(D)] for r in range(D)]


def pack(slabs, B, M, D, cap, fill_bits, fill_int, cols=COSTATE, phi=True):
    """What the call must leave in buffers filled with fill_bits / fill_int: (tq[B][M][cap], det[B][M][cap]) as uint64 views,
    count[B][M], nchange[B][M], tconj[B][M] (uint64), Phi[B][M][S][C] (uint64; None with phi=False).  slabs[b][i]."""
    S = 2 * D
    C = S if cols == ALL else D
    tq = np.full((B, M, cap), np.uint64(fill_bits), dtype=np.uint64)
    det = tq.copy()
    count = np.full((B, M), fill_int, dtype=np.int32)
    nchange = count.copy()
    tconj = np.full((B, M), np.uint64(fill_bits), dtype=np.uint64)
    Phi = np.full((B, M, S, C), np.uint64(fill_bits), dtype=np.uint64) if phi else None
    for b in range(B):
        for i in range(M):
            s = slabs[b][i]
            k = min(s["count"], cap)
            tq[b, i, :k] = np.array(s["tq"][:k], dtype=np.float64).view(np.uint64)
            det[b, i, :k] = np.array(s["det"][:k], dtype=np.float64).view(np.uint64)
            count[b, i], nchange[b, i] = s["count"], s["nchange"]
            tconj[b, i] = np.array([s["tconj"]], dtype=np.float64).view(np.uint64)[0]
            if phi:
                Phi[b, i] = np.ascontiguousarray(s["phi"], dtype=np.float64).view(np.uint64)
    return tq, det, count, nchange, tconj, Phi
