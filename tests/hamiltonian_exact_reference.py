"""The definitions of NESTED DUAL NUMBERS, of socp_hamiltonian_jacobian_batch and of plugin::FromHamiltonianExact (include/socp_hip.h,
"NESTED DUAL NUMBERS"; socp_amd/csrc/dualn.hpp, hamiltonian_model.hpp) restated in Python, one IEEE operation per line (helper of
test_hamiltonian_exact_cpu.py, test_gpu_hamiltonian_exact.py and tools/hamiltonian_exact_timing.py, not a test), on top of
tests/fields_reference.py (its Dual and kits), tests/exact_jacobian_reference.py (the generic-kit Hamiltonian texts, which run on the
nested number unchanged), tests/sensitivity_reference.py and tests/hamiltonian_model_reference.py.

A `Nested` is (v; d[0 .. W)) whose parts are fields_reference.Dual objects -- Python floats (IEEE doubles: the kernels must reproduce
every bit) or 240-bit mpmath numbers inside (fields_reference.DualMpf).  Every listed operation of a rule is ONE operation of the inner
Dual, with that class's own roundings.  The derivative part of an inner Dual may be a numpy array: the columns of a Jacobian, the
directions of a sensitivity call or the columns of a field then travel together, as in the references this one builds on -- the value
parts of all of them are the same numbers and numpy's elementwise operations are the scalar IEEE ones.

`mutate` names the WRONG restatements the CPU tests must catch: "outer_shifted" (the outer seed e_j placed on X[j + 1]),
"drop_inner_cross" (in the nested product's l = a.d[k] b.v the inner term a.d[k].d b.v.v dropped), "sqrt_inner_of_s" (d_sqrt's part k
keeps the value of a.d[k] / (s + s) but takes its inner derivative from s), "plain_param" (a plain dual parameter's inner derivative
part dropped where it meets a nested number -- visible in a parameter sensitivity only).

dint_hx / osc1d_hx (tests/plugin/dint_hx_plugin.hip, osc1d_hx_plugin.hip) are models whose right-hand side over dual numbers IS the
nested gradient: `entries()` lends them to fields_reference, exact_jacobian_reference and sensitivity_reference for the length of a
call."""
import contextlib

import numpy as np

import exact_jacobian_reference as ejr
import fields_reference as fr
import hamiltonian_model_reference as hm
from fields_reference import Dual, DualKit, DualMpfKit, HAVE_MPMATH, mpf, mpmath   # noqa: F401

MUTATIONS = ("outer_shifted", "drop_inner_cross", "sqrt_inner_of_s", "plain_param")
BASE = {"dint_hx": "dint", "osc1d_hx": "osc1d"}           # the model whose Hamiltonian text an exact H-only model carries
WIDTH = {"dint_hx": 2, "osc1d_hx": 1}                      # their pass width on dual numbers (it changes no bit)
HAMILTONIAN = dict(ejr.HAMILTONIAN)
HAMILTONIAN.update({name: ejr.HAMILTONIAN[base] for name, base in BASE.items()})


def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


def _zero_like(d):
    """+0.0 in the shape and carrier of an inner derivative part."""
    if isinstance(d, np.ndarray):
        return np.array([type(x)(0.0) for x in d.ravel()], dtype=d.dtype).reshape(d.shape) if d.dtype == object else np.zeros_like(d)
    return type(d)(0.0)


class Nested(Dual):
    """(v; d[0 .. W)), every part an inner Dual.  A subclass of Dual so that Python tries THIS class's reflected operation first when
    a plain inner Dual (a parameter) stands on the left."""
    __slots__ = ()
    MUTATE = None

    def _plain(self, c):
        """A plain number beside a nested one: a carrier number, or an inner Dual (plain at the outer level only)."""
        assert not isinstance(c, Nested)
        if self.MUTATE == "plain_param" and isinstance(c, Dual):
            return c.v
        return c

    def __neg__(self):
        v = -self.v
        return self._new(v, [-dk for dk in self.d])

    def __abs__(self):
        v = abs(self.v)
        flip = ValueKit.value(self.v) < 0
        return self._new(v, [-dk if flip else dk for dk in self.d])

    def __add__(self, o):
        if isinstance(o, Nested):
            v = self.v + o.v
            return self._new(v, [a + b for a, b in zip(self.d, o.d)])
        c = self._plain(o)
        v = self.v + c
        return self._new(v, list(self.d))

    def __radd__(self, o):
        c = self._plain(o)
        v = c + self.v
        return self._new(v, list(self.d))

    def __sub__(self, o):
        if isinstance(o, Nested):
            v = self.v - o.v
            return self._new(v, [a - b for a, b in zip(self.d, o.d)])
        c = self._plain(o)
        v = self.v - c
        return self._new(v, list(self.d))

    def __rsub__(self, o):
        c = self._plain(o)
        v = c - self.v
        return self._new(v, [-dk for dk in self.d])

    def __mul__(self, o):
        if isinstance(o, Nested):
            v = self.v * o.v
            d = []
            for ak, bk in zip(self.d, o.d):
                left = ak * o.v
                if self.MUTATE == "drop_inner_cross":
                    left = type(ak)(ak.v * o.v.v, ak.v * o.v.d)
                right = self.v * bk
                d.append(left + right)
            return self._new(v, d)
        c = self._plain(o)
        v = self.v * c
        return self._new(v, [dk * c for dk in self.d])

    def __rmul__(self, o):
        c = self._plain(o)
        v = c * self.v
        return self._new(v, [c * dk for dk in self.d])

    def __truediv__(self, o):
        if isinstance(o, Nested):
            q = self.v / o.v
            d = []
            for ak, bk in zip(self.d, o.d):
                m = q * bk
                num = ak - m
                d.append(num / o.v)
            return self._new(q, d)
        c = self._plain(o)
        v = self.v / c
        return self._new(v, [dk / c for dk in self.d])

    def __rtruediv__(self, o):
        c = self._plain(o)
        q = c / self.v
        d = []
        for ak in self.d:
            m = q * ak
            neg = -m
            d.append(neg / self.v)
        return self._new(q, d)

    def sqrt(self):
        s = self.v.sqrt()
        if ValueKit.value(s) == 0:
            return self._new(s, [type(s)(type(s.v)(0.0), _zero_like(s.d)) for _ in self.d])
        s2 = s + s
        d = []
        for ak in self.d:
            q = ak / s2
            if self.MUTATE == "sqrt_inner_of_s":
                q = type(q)(q.v, s.d)
            d.append(q)
        return self._new(s, d)

    def exp(self):
        e = self.v.exp()
        return self._new(e, [e * dk for dk in self.d])


_MUTANTS = {None: Nested}
for _m in ("drop_inner_cross", "sqrt_inner_of_s", "plain_param"):
    _MUTANTS[_m] = type("Nested_" + _m, (Nested,), {"__slots__": (), "MUTATE": _m})


class ValueKit:
    @staticmethod
    def value(x):
        """The innermost value: what a comparison reads."""
        while isinstance(x, Dual):
            x = x.v
        return x


class NestedKit(DualKit):
    """Nested numbers, inner Duals and plain numbers side by side (DualKit's sqrt / exp dispatch on the number itself); decisions read
    the innermost value."""
    value = staticmethod(ValueKit.value)


class NestedMpfKit(DualMpfKit):
    value = staticmethod(ValueKit.value)


def nested_gradient(model, P, sw, t, X, width=None, mutate=None):
    """symplectic_gradient<Mdl, W, Dual>: X[S] inner Duals (any Dual class, derivative parts scalars or arrays) -> G[S] inner Duals.
    P may hold inner Duals (the dual view of a parameter block); sw and t are plain carrier numbers."""
    Hfn = HAMILTONIAN[model]
    S = len(X)
    D = S // 2
    W = S if width is None else int(width)
    assert 1 <= W <= S
    inner = type(X[0])
    high = _is_high(ValueKit.value(X[0]))
    K = NestedMpfKit() if high else NestedKit()
    cls = _MUTANTS[mutate if mutate in _MUTANTS else None]
    num = type(X[0].v)
    one = lambda: inner(num(1.0), _zero_like(X[0].d))                                      # noqa: E731  T(1.0) = (1.0, +0.0)
    zero = lambda: inner(num(0.0), _zero_like(X[0].d))                                     # noqa: E731  T(0.0) = (0.0, +0.0)
    dH = [None] * S
    for q in range(0, S, W):
        Y = [cls(X[i], [one() if i == q + k else zero() for k in range(W)]) for i in range(S)]
        with np.errstate(all="ignore"):
            H = Hfn(K, list(P), list(sw), t, Y)
        for k in range(W):
            if q + k < S:
                dH[q + k] = H.d[k]
    G = [None] * S
    for i in range(D):
        G[i] = dH[i + D]
        G[i + D] = -dH[i]
    return G


def hamiltonian_jacobian(model, P, sw, t, X, width=None, high=False, mutate=None):
    """(A, G) at one point: A[i][j] = dG_i/dX_j (S x S: a float64 array, or dtype object in 240 bits) and the value parts G[S].  The S
    outer directions travel together as the entries of the inner derivative arrays.  width: the derivative parts of one inner pass
    (default S); X may hold mpf numbers with high=True."""
    assert mutate is None or mutate in MUTATIONS
    S = len(X)
    inner = fr.DualMpf if high else Dual
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
    shift = 1 if mutate == "outer_shifted" else 0
    Pn, swn, tn = [num(p) for p in P], [num(s) for s in sw], num(t)
    Xd = [inner(num(X[i]), np.array([num(1.0) if (i + shift) % S == j else num(0.0) for j in range(S)], dtype=object if high else np.float64))
          for i in range(S)]
    Gd = nested_gradient(model, Pn, swn, tn, Xd, width=width, mutate=mutate)
    A = np.array([[g.d[j] for j in range(S)] for g in Gd], dtype=object if high else np.float64)
    G = [g.v for g in Gd]
    return A, (G if high else np.array(G, dtype=np.float64))


def hamiltonian_jacobian_batch(model, P, t, X, sw=None, sw_default=(0.0, 0.0), width=None):
    """What the call leaves, in doubles: (A[B][S * S] COLUMN-major per point, G[B][S]).  sw[B][2] or None: the context's switching
    times sw_default."""
    X = np.asarray(X, dtype=np.float64)
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (X.shape[0],))
    As, Gs = [], []
    for b in range(X.shape[0]):
        A, G = hamiltonian_jacobian(model, P, sw_default if sw is None else sw[b], t[b], X[b], width=width)
        As.append(np.ascontiguousarray(A.T).ravel())
        Gs.append(G)
    return np.array(As), np.array(Gs)


# ---- the exact H-only models' right-hand sides over a generic kit: the (nested) gradient of the base model's Hamiltonian text -------

MUTATE_RHS = [None]                                        # the mutation the lent right-hand sides run with (tests set and reset it)


def _hx_rhs(model):
    def rhs(K, P, sw, t, X):
        if isinstance(X[0], Dual):
            return nested_gradient(model, P, sw, t, X, width=WIDTH[model], mutate=MUTATE_RHS[0]), None, None
        return hm.symplectic_gradient(BASE[model], P, sw, t, X, width=WIDTH[model], high=_is_high(X[0])), None, None
    rhs.__name__ = model + "_ref"
    rhs.__doc__ = ("tests/plugin/%s_plugin.hip: rhs_t = symplectic_gradient of %s's Hamiltonian text on the carrier of X.  "
                   "Returns (Xdot[S], None, None)." % (model, BASE[model]))
    return rhs


RHS = dict(fr.RHS)
RHS.update({name: _hx_rhs(name) for name in BASE})
SWITCHING_READS_XP = dict(ejr.SWITCHING_READS_XP)
SWITCHING_READS_XP.update({name: True for name in BASE})      # FromHamiltonianExact's default row H(t, X-) - H(t, X+)


@contextlib.contextmanager
def entries():
    """fields_reference, exact_jacobian_reference and sensitivity_reference look their models up in fields_reference.RHS (one dict,
    imported by all three) and in exact_jacobian_reference's HAMILTONIAN / SWITCHING_READS_XP: lend them this module's entries for the
    length of a call, and take them back."""
    tables = ((fr.RHS, RHS), (ejr.HAMILTONIAN, HAMILTONIAN), (ejr.SWITCHING_READS_XP, SWITCHING_READS_XP))
    for theirs, ours in tables:
        for name in BASE:
            theirs[name] = ours[name]
    try:
        yield
    finally:
        for theirs, _ in tables:
            for name in BASE:
                theirs.pop(name, None)


def plain_rhs(model, P, sw, t, X):
    """The restated right-hand side on Python floats: an array."""
    return np.array(fr.rhs_on(RHS[model], fr.PlainKit(), [float(p) for p in P], [float(s) for s in sw], float(t), [float(x) for x in X]))
