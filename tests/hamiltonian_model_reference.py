"""The definition of socp_hamiltonian_gradient_batch and of plugin::FromHamiltonian (include/socp_hip.h, "HAMILTONIAN GRADIENT";
socp_amd/csrc/hamiltonian_model.hpp) restated in Python, one IEEE operation per line (helper of test_hamiltonian_model_cpu.py,
test_gpu_hamiltonian_model.py and tools/hamiltonian_model_timing.py, not a test), on top of tests/fields_reference.py -- its Dual
with numpy arrays as derivative parts -- and the generic-kit Hamiltonians of tests/exact_jacobian_reference.py.

symplectic_gradient seeds X[i] = (X[i], e_i), runs the model's Hamiltonian text in ceil(S / W) passes of W derivative parts and
returns G[i] = H.d[i + D], G[i + D] = -H.d[i].  Two carriers: Python floats (IEEE doubles -- the kernel must reproduce every bit) and
mpmath numbers (240 bits; X may then hold mpf numbers).  `mutate` names the WRONG restatements the CPU tests must catch:
"not_swapped" (G = (dH/dx, -dH/dp)), "no_minus" (G = (dH/dp, +dH/dx)), "shifted" (X[i] seeded with e_{i+1}).

dint_h / osc1d_h (tests/plugin/dint_h_plugin.hip, osc1d_h_plugin.hip) are models whose right-hand side IS that gradient: their
entries live in the RHS / HAMILTONIAN tables HERE; `entries()` lends them to exact_jacobian_reference for the length of a call."""
import contextlib

import numpy as np

import exact_jacobian_reference as ejr
import fields_reference as fr
from fields_reference import Dual, DualKit, DualMpfKit, HAVE_MPMATH, mpf, mpmath   # noqa: F401

MUTATIONS = ("not_swapped", "no_minus", "shifted")
BASE = {"dint_h": "dint", "osc1d_h": "osc1d"}             # the model whose Hamiltonian text an H-only model carries
HAMILTONIAN = dict(ejr.HAMILTONIAN)
HAMILTONIAN.update({name: ejr.HAMILTONIAN[base] for name, base in BASE.items()})


def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


def symplectic_gradient(model, P, sw, t, X, width=None, high=False, mutate=None):
    """G[S] at one point: floats, or mpf numbers with high=True.  width: the derivative parts of one pass (default S, one pass);
    directions at or beyond S are seeded with zeros and dropped."""
    assert mutate is None or mutate in MUTATIONS
    Hfn = HAMILTONIAN[model]
    S = len(X)
    D = S // 2
    W = S if width is None else int(width)
    assert 1 <= W <= S
    cls, K = (fr.DualMpf, DualMpfKit()) if high else (Dual, DualKit())
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
    Pn, swn, tn, Xn = [num(p) for p in P], [num(s) for s in sw], num(t), [num(x) for x in X]
    shift = 1 if mutate == "shifted" else 0
    dH = [None] * S
    for q in range(0, S, W):
        Y = [cls(Xn[i], np.array([num(1.0) if (i + shift) % S == q + k else num(0.0) for k in range(W)], dtype=object if high else np.float64))
             for i in range(S)]
        with np.errstate(all="ignore"):
            H = Hfn(K, list(Pn), list(swn), tn, Y)
        for k in range(W):
            if q + k < S:
                dH[q + k] = H.d[k] if high else float(H.d[k])
    G = [None] * S
    for i in range(D):
        if mutate == "not_swapped":
            G[i], G[i + D] = dH[i], -dH[i + D]
        elif mutate == "no_minus":
            G[i], G[i + D] = dH[i + D], dH[i]
        else:
            G[i], G[i + D] = dH[i + D], -dH[i]
    return G


def gradient_batch(model, P, t, X, sw=None, sw_default=(0.0, 0.0), width=None):
    """What the call leaves in G[B][S], in doubles.  sw[B][2] or None: the context's switching times sw_default."""
    X = np.asarray(X, dtype=np.float64)
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (X.shape[0],))
    return np.array([symplectic_gradient(model, P, sw_default if sw is None else sw[b], t[b], X[b], width=width) for b in range(X.shape[0])])


def plain_hamiltonian(model, P, sw, t, X):
    """hamiltonian_t<double> on Python floats."""
    return HAMILTONIAN[model](fr.PlainKit(), [float(p) for p in P], [float(s) for s in sw], float(t), [float(x) for x in X])


# ---- the H-only models' right-hand sides over a generic kit: the gradient of the base model's Hamiltonian text --------------------

def _h_rhs(model):
    def rhs(K, P, sw, t, X):
        vals = [K.value(x) for x in X]
        G = symplectic_gradient(model, P, sw, t, vals, high=_is_high(vals[0]))
        return G, None, None
    rhs.__name__ = model + "_ref"
    rhs.__doc__ = "tests/plugin/%s_plugin.hip: Xdot = symplectic_gradient of %s's Hamiltonian text.  Returns (Xdot[S], None, None)." % (model, BASE[model])
    return rhs


RHS = dict(fr.RHS)
RHS.update({name: _h_rhs(name) for name in BASE})
SWITCHING_READS_XP = dict(ejr.SWITCHING_READS_XP)
SWITCHING_READS_XP.update({name: True for name in BASE})      # FromHamiltonian's default row H(t, X-) - H(t, X+)


def plain_rhs(model, P, sw, t, X):
    """The restated right-hand side on Python floats: an array (fields_reference.plain_rhs over this module's table)."""
    return np.array(fr.rhs_on(RHS[model], fr.PlainKit(), [float(p) for p in P], [float(s) for s in sw], float(t), [float(x) for x in X]))


def rhs_high(model, P, sw, t, X):
    """The restated right-hand side in 240 bits: a list of mpf numbers; X may hold mpf numbers."""
    num = lambda x: x if _is_high(x) else mpf(float(x))                                   # noqa: E731
    return [mpf(q) for q in fr.rhs_on(RHS[model], DualMpfKit(), [num(p) for p in P], [num(s) for s in sw], num(t), [num(x) for x in X])]


@contextlib.contextmanager
def entries():
    """exact_jacobian_reference looks its models up in its own tables: lend it this module's H-only entries for the length of a
    call, and take them back."""
    tables = ((ejr.RHS, RHS), (ejr.HAMILTONIAN, HAMILTONIAN), (ejr.SWITCHING_READS_XP, SWITCHING_READS_XP))
    for theirs, ours in tables:
        for name in BASE:
            theirs[name] = ours[name]
    try:
        yield
    finally:
        for theirs, _ in tables:
            for name in BASE:
                theirs.pop(name, None)


def residual_row(model, P, sw, prob, z, N):
    """The shooting function of one row in doubles: exact_jacobian_row(..., derivs=False) on this module's RHS entry."""
    with entries():
        return ejr.exact_jacobian_row(model, P, sw, prob, z, N, derivs=False)[1]


def rk4(model, P, sw, t, X, h):
    """One RK4 step on Python floats in the association order of odeTools.cpp:89-98 (fields_reference.rk4_dual's, on plain numbers)."""
    f = lambda tt, Y: list(plain_rhs(model, P, sw, tt, Y))                                # noqa: E731
    h2 = h / 2.0
    th = t + h / 2.0
    F1 = f(t, X)
    F2 = f(th, [x + h2 * k for x, k in zip(X, F1)])
    F3 = f(th, [x + h2 * k for x, k in zip(X, F2)])
    F4 = f(t + h, [x + h * k for x, k in zip(X, F3)])
    h6 = h / 6.0
    return [x + h6 * (k1 + (k4 + 2.0 * (k2 + k3))) for x, k1, k2, k3, k4 in zip(X, F1, F2, F3, F4)]


def integrate(model, P, sw, t1, t2, X0, N, rhs=None, high=False):
    """Lane::integrate's fixed-step loop (the step sequence decided in doubles, as fields_reference.fields_segment does) on Python
    floats; returns the list of states after every step.  rhs / high: another right-hand side (K-generic) and the 240-bit carrier,
    for the recurrences' own truth."""
    t1, t2 = float(t1), float(t2)
    dt = (t2 - t1) / N
    t, guard = t1, N + 8
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
    X = [num(x) for x in X0]
    Pn, swn = [num(p) for p in P], [num(s) for s in sw]
    K = DualMpfKit() if high else fr.PlainKit()
    fn = rhs if rhs is not None else RHS[model]
    f = lambda tt, Y: fr.rhs_on(fn, K, Pn, swn, num(tt), Y)                               # noqa: E731
    out = []
    while t < (t2 - dt / 2) and guard > 0:
        guard -= 1
        h = num((t2 - t) if (t + dt > t2) else dt)
        h2 = h / 2.0
        th = num(t) + h / 2.0
        F1 = f(t, X)
        F2 = f(th, [x + h2 * k for x, k in zip(X, F1)])
        F3 = f(th, [x + h2 * k for x, k in zip(X, F2)])
        F4 = f(num(t) + h, [x + h * k for x, k in zip(X, F3)])
        h6 = h / 6.0
        X = [x + h6 * (k1 + (k4 + 2.0 * (k2 + k3))) for x, k1, k2, k3, k4 in zip(X, F1, F2, F3, F4)]
        out.append(list(X))
        t = t + dt
    return out
