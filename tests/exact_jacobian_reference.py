"""The definition of socp_exact_jacobian_batch (include/socp_hip.h) restated in Python, one IEEE operation per line (helper of
test_exact_jacobian_cpu.py and test_gpu_exact_jacobian.py, not a test), on top of tests/fields_reference.py: its Dual, DualKit and
DualMpfKit and the generic-kit right-hand sides.

The S + 1 columns of a segment travel together: one state whose derivative parts are numpy arrays of S + 1 entries -- the value
parts of all columns are the same numbers and numpy's elementwise products, sums and quotients are the scalar IEEE operations.
Entry S of those arrays is the LENGTH column.  Two carriers: Python floats (IEEE doubles -- the kernel must reproduce every
output bit for bit) and mpmath numbers (arrays of dtype object: the 240-bit truth of the same recurrence, where the unknowns may
be 240-bit numbers themselves, so the value parts are the 240-bit residual).

`mutate` names the WRONG restatements the CPU tests must catch: "no_length" (the length column dropped), "no_minus_identity" (the
-I of the next block missing), "no_ci" (the weight c(i, f) left out of w), "drop_hd_length" (h F with the term h.d F.v dropped in
the length lane only)."""
import numpy as np

import fields_reference as fr
from fields_reference import Dual, DualKit, DualMpfKit, RHS, rhs_on, _as_dual, HAVE_MPMATH, mpf, mpmath   # noqa: F401
from fast_reference import goddard_ref

FIXED, FREE, CONTINUOUS = 0, 1, 2
MUTATIONS = ("no_length", "no_minus_identity", "no_ci", "drop_hd_length")


# ---- the Hamiltonians over a generic kit (hamiltonian_t of models_exact.hpp; Goddard's is fast_reference.goddard_ref's H) ---------

def goddard_hamiltonian_ref(K, P, sw, t, X):
    return goddard_ref(K, P, sw, t, X)[2]


def dint_hamiltonian_ref(K, P, sw, t, X):
    """Reference operation order (oracle/socp_oracle.c: dint_control, dint_hamiltonian).  P = u_max, a_max, muT."""
    u_max, a_max, muT = P[0], P[1], P[2]
    u = [-X[9] / a_max, -X[10] / a_max, -X[11] / a_max]
    norm_c = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    if K.cmp("|u|-umax", norm_c - u_max, ">"):
        u = [ui / norm_c*u_max for ui in u]
    norm_u = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    return (muT + a_max * a_max*norm_u*norm_u / 2 + X[6] * X[3] + X[7] * X[4] + X[8] * X[5]
            + a_max * (X[9]*u[0] + X[10] * u[1] + X[11] * u[2]))


def covid_hamiltonian_ref(K, P, sw, t, X):
    """Reference operation order (oracle/socp_oracle.c: covid_control, covid_hamiltonian)."""
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
        Ipen = muI*(I - Imax)*(I - Imax) / 2
    return (u*u / 2 + Ipen
            + pS * (-Rt / Tinf / N*S*I)
            + pE * (Rt / Tinf / N*S*I - E / Tinc)
            + pI * (E / Tinc - I / Tinf)
            + pR * (I / Tinf))


def osc1d_hamiltonian_ref(K, P, sw, t, X):
    """tests/plugin/osc1d_exact_jacobian_plugin.hip."""
    u = -X[1]
    return u * u / 2 - P[0] * X[0] * X[0] / 2 + X[1] * u


HAMILTONIAN = {"goddard": goddard_hamiltonian_ref, "dint": dint_hamiltonian_ref, "covid": covid_hamiltonian_ref, "osc1d": osc1d_hamiltonian_ref}
SWITCHING_READS_XP = {"goddard": False, "dint": True, "covid": True, "osc1d": True}      # trait kSwitchingReadsXp


def hamiltonian_on(model, K, P, sw, t, X):
    return HAMILTONIAN[model](K, list(P), list(sw), t, list(X))


def switching_on(model, K, P, sw, t, X, Xp):
    """switching_fn_t: H(t, X) for Goddard (goddard.cpp:343-370), the default H(t, X) - H(t, Xp) otherwise (model.hpp:299-304)."""
    H = hamiltonian_on(model, K, P, sw, t, X)
    return H - hamiltonian_on(model, K, P, sw, t, Xp) if SWITCHING_READS_XP[model] else H


def plain_hamiltonian(model, P, sw, t, X):
    """hamiltonian_t on Python floats (PlainKit)."""
    return hamiltonian_on(model, fr.PlainKit(), [float(p) for p in P], [float(s) for s in sw], float(t), [float(x) for x in X])


def plain_switching(model, P, sw, t, X, Xp):
    return switching_on(model, fr.PlainKit(), [float(p) for p in P], [float(s) for s in sw], float(t), [float(x) for x in X], [float(x) for x in Xp])


# ---- the layout of socp_problem_set ---------------------------------------------------------------------------------------------

class Layout:
    """node_kind (>= 0: index of the free time's unknown, -1 FIXED, -2 interpolated between lo and hi), ft_row, sw_node0 / 1, n."""

    def __init__(self, prob):
        M, S = prob.M, 2 * prob.dim
        self.M, self.S, self.D = M, S, prob.dim
        self.kind, self.ft_row, self.lo, self.hi = [-2] * (M + 1), [-1] * (M + 1), [0] * (M + 1), [0] * (M + 1)
        nbr, sw_nodes = S * M, []
        for j in range(M + 1):
            if prob.mode_t[j] == FIXED:
                self.kind[j] = -1
            if prob.mode_t[j] == FREE:
                self.kind[j] = self.ft_row[j] = nbr
                nbr += 1
                if j < M:
                    sw_nodes.append(j)
        self.n = nbr
        self.sw_node = (sw_nodes + [-1, -1])[:2]
        cur = 0
        for j in range(M + 1):
            if self.kind[j] != -2:
                for k in range(cur + 1, j):
                    self.lo[k], self.hi[k] = cur, j
                self.lo[j] = self.hi[j] = j
                cur = j


def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


def exact_jacobian_row(model, P, sw, prob, z, N, high=False, derivs=True, mutate=()):
    """One row of the batch: (J, F) with J[row][col] = dF_row / dz_col (an n x n array: float64, or dtype object in 240 bits) and
    F[n].  high: the same recurrence in 240 bits; z may then hold mpf numbers.  derivs=False: the value parts alone (the residual)."""
    assert set(mutate) <= set(MUTATIONS)
    fn, lay = RHS[model], Layout(prob)
    M, S, D, n = lay.M, lay.S, lay.D, lay.n
    K = DualMpfKit() if high else DualKit()
    cls = fr.DualMpf if high else Dual
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
    G = S + 1 if derivs else 0
    vec = lambda vals: np.array([num(v) for v in vals], dtype=object if high else np.float64)      # noqa: E731
    zero = vec([0.0] * G)
    zz, Pn = [num(v) for v in z], [num(p) for p in P]
    xn = [[num(v) for v in row] for row in prob.xnode]
    J = np.array([[num(0.0)] * n for _ in range(n)], dtype=object if high else np.float64).reshape(n, n)
    F = [num(0.0)] * n

    # Timeline::nt / switching_time
    jt = lambda j: zz[lay.kind[j]] if lay.kind[j] >= 0 else num(prob.time[j])                       # noqa: E731

    def nt(k):
        if lay.kind[k] >= -1:
            return jt(k)
        a, b = lay.lo[k], lay.hi[k]
        ta, tb = jt(a), jt(b)
        return ta + (k - a) * (tb - ta) / (b - a)

    sws = [nt(node) if node >= 0 else num(dflt) for node, dflt in zip(lay.sw_node, sw)]

    def weight(j, f):
        """c(j, f)"""
        if j == f:
            return num(1.0)
        if lay.kind[j] != -2:
            return num(0.0)
        a, b = lay.lo[j], lay.hi[j]
        q = num(j - a) / num(b - a)
        return q if f == b else (num(1.0) - q if f == a else num(0.0))

    def hmul(h, Fk):
        """h F by the full dual x dual rule (the mutation drops h.d F.v in the length lane)"""
        out = h * Fk
        if "drop_hd_length" in mutate and derivs:
            d = out.d.copy()
            d[S] = (h.v * Fk.d)[S]
            out = cls(out.v, d)
        return out

    def rk4(t, X, h):
        f = lambda tt, Y: [_as_dual(cls, q, zero) for q in rhs_on(fn, K, Pn, sws, tt, Y)]          # noqa: E731
        h2 = h / 2.0
        th = t + h / 2.0
        F1 = f(t.v, X)
        Y = [x + hmul(h2, k) for x, k in zip(X, F1)]
        F2 = f(th.v, Y)
        Y = [x + hmul(h2, k) for x, k in zip(X, F2)]
        F3 = f(th.v, Y)
        Y = [x + hmul(h, k) for x, k in zip(X, F3)]
        Fs = [a + b for a, b in zip(F2, F3)]
        te = t + h
        F4 = f(te.v, Y)
        h6 = h / 6.0
        return [x + hmul(h6, k1 + (k4 + 2.0 * ks)) for x, k1, k4, ks in zip(X, F1, F4, Fs)]

    for i in range(M):
        t1, t2 = nt(i), nt(i + 1)
        first = S * i
        X = [cls(zz[first + j], vec([1.0 if c == j else 0.0 for c in range(G)])) for j in range(S)]

        def put_state(row, e):
            if derivs:
                J[row, first:first + S] = e.d[:S]

        # ---- the rows on the START state
        if i == 0:
            for j in range(D):
                e = X[j + D] if prob.mode_x[0][j] == FREE else X[j] - xn[0][j]
                put_state(j, e)
                F[j] = e.v
            if lay.ft_row[0] >= 0:
                H = hamiltonian_on(model, K, Pn, sws, t1, X)
                put_state(lay.ft_row[0], H)
                F[lay.ft_row[0]] = H.v
        elif derivs:
            for c in range(S):
                if prob.mode_x[i][c % D] == FIXED:
                    if c < D:
                        J[first + D + c, first + c] = num(1.0)
                elif "no_minus_identity" not in mutate:
                    J[first + c, first + c] = num(-1.0)
            if SWITCHING_READS_XP[model] and lay.ft_row[i] >= 0:
                put_state(lay.ft_row[i], -hamiltonian_on(model, K, Pn, sws, t1, X))

        # ---- the loop of Lane::integrate on duals
        with np.errstate(all="ignore"):
            t2d = cls(t2, vec([0.0] * S + [1.0]) if derivs else zero)
            t = cls(t1, zero)
            dt = (t2d - t) / N
            guard = N + 8
            while t.v < (t2 - dt.v / 2) and guard > 0:
                guard -= 1
                step = (t2d - t) if (t.v + dt.v > t2) else dt
                X = rk4(t, X, step)
                t = t + dt

        # ---- the free times the segment's length depends on
        A = lay.lo[i] if lay.kind[i] == -2 else i
        Bn = lay.hi[i + 1] if lay.kind[i + 1] == -2 else i + 1
        frees = []
        for f in (A, Bn):
            if lay.kind[f] >= 0 and "no_length" not in mutate:
                w = weight(i + 1, f) - (num(0.0) if "no_ci" in mutate else weight(i, f))
                if w != 0:
                    frees.append((lay.kind[f], w))

        def emit(row, e, deriv=True):
            F[row] = e.v
            if deriv and derivs:
                put_state(row, e)
                with np.errstate(all="ignore"):
                    for k, w in frees:
                        J[row, k] = w * e.d[S]

        # ---- the rows on the END state
        with np.errstate(all="ignore"):
            if i < M - 1:
                Xp = zz[S * (i + 1):S * (i + 2)]
                if lay.ft_row[i + 1] >= 0:
                    emit(lay.ft_row[i + 1], switching_on(model, K, Pn, sws, t2, X, [cls(x, zero) for x in Xp]))
                for j in range(D):
                    row = S * (i + 1) + j
                    fixed = prob.mode_x[i + 1][j] == FIXED
                    xdj = xn[i + 1][j]
                    emit(row, X[j] - (xdj if fixed else Xp[j]))
                    if fixed:
                        F[row + D] = Xp[j] - xdj
                    else:
                        emit(row + D, X[j + D] - Xp[j + D])
            if i == M - 1:
                for j in range(D):
                    emit(D + j, X[j + D] if prob.mode_x[M][j] == FREE else X[j] - xn[M][j])
                if lay.ft_row[M] >= 0:
                    emit(lay.ft_row[M], hamiltonian_on(model, K, Pn, sws, t2, X))
    return J, (F if high else np.array(F, dtype=np.float64))


def exact_jacobian_batch(model, P, sw, prob, Z, N, blocks=None):
    """What the call leaves: (Fjac[B][n*n] COLUMN-major, F[B][n]) in doubles.  blocks = (params[B][nparams + 2], time[B][M+1],
    xnode[B][(M+1) 2d]), any of them None: row b's own parameters (then two switching times), times and node states."""
    from oracle.oracle import Problem
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    Js, Fs = [], []
    for b, z in enumerate(Z):
        Pb = P if pp is None else pp[b][:len(P)]
        swb = sw if pp is None else pp[b][len(P):len(P) + 2]
        pb = prob if tt is None and xx is None else Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time if tt is None else tt[b],
                                                             prob.xnode if xx is None else xx[b])
        J, F = exact_jacobian_row(model, Pb, swb, pb, z, N)
        Js.append(np.ascontiguousarray(J.T).ravel())
        Fs.append(F)
    return np.array(Js), np.array(Fs)
