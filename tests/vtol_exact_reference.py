"""vtolUAV in the exact-derivative stack, restated in Python one IEEE operation per line (helper of test_vtol_exact_cpu.py,
test_gpu_vtol_exact.py, golden/make_vtol_exact_golden.py and tools/vtol_exact_timing.py, not a test): the model's texts over a
number type (socp_amd/csrc/models_vtol.hpp: control_t, map_exact_t, rhs_t, hamiltonian_t, switching_fn_t, final_row_t,
switching_state_t) on the dual numbers of fields_reference.py with the tanh rule added, and the definition of
socp_exact_jacobian_batch (include/socp_hip.h) with the two hooks: custom final rows and the switching_state rows of a FREE state
component of an interior node.

The texts below (control_t ... hamiltonian_t) are vtol_reference.vtol_ref written the way the texts over T are written: the running sums of the map start as the NUMBER
zero (value and derivative +0.0), the NaN reset tests the value part and zeroes the whole number, phi*g + psi*0.0 adds a plain
zero.  vtol_ref itself decides a NaN on the inputs and resets to a plain constant, which gives the same values and the same
derivatives as numbers but not the same sign of a zero derivative.  The tie to the reference is on the value parts:
in numpy.float64 they equal vtol_ref on F64Kit bit for bit (test_vtol_exact_cpu.py asserts it on every state it uses).

Two carriers, as in exact_jacobian_reference.py: numpy.float64 (the S + 1 columns of a segment travel together, the derivative
parts are arrays of S + 1 doubles) and mpmath numbers (arrays of dtype object: the 240-bit truth of the same recurrence).  In
doubles tanh is numpy's; the device library's differs from it in the last places, which is why the kernel is held to the 240-bit
matrix and not to these bits wherever a tanh is evaluated (an EMPTY map evaluates none: there every bit must agree).

ROW AND COLUMN LAYOUT (beyond exact_jacobian_reference.py's).  Last node: row D + j is final_row_t(j, mode, X, xd) on the dual end
state -- X[j + D] - invSigmaXwp (nWP_tot - nWP) (X[j] - xd[j]) - 0.02 (X[j] - xd[j]) when FREE, X[j] - xd[j] otherwise -- and the
free-final-time row is H + final_h_offset.  Interior node k, component j FREE: rows S k + j and S k + D + j are
fs = X[j] - Xp[j] and fc = (X[j + D] - Xp[j + D]) - invSigmaXwp (X[j] - xd[j]), differentiated with respect to the arriving
segment's columns (and its free times through the length column) from its dual end state X; the columns of the node's own unknowns
Xp hold exactly -1 at (S k + j, S k + j) and at (S k + D + j, S k + D + j), the entries of a CONTINUOUS row
(kSwitchingStateXpContinuous).

`mutate` names the WRONG restatements the CPU test must catch: "tanh_no_factor" ((1 - th^2) dropped from the tanh rule),
"hook_no_inv_sigma" (the invSigmaXwp term of the hook dropped), "final_no_wp_weight" / "final_no_002" (a term of final_row dropped),
"hook_no_minus_one" (the -1 of the next segment's columns missing on hook rows), "no_length" (the length column dropped)."""
import numpy as np

import fields_reference as fr
import vtol_reference as vr
from exact_jacobian_reference import Layout, FIXED, FREE, CONTINUOUS    # noqa: F401
from fast_reference import F64, F64Kit, HAVE_MPMATH, mpf, mpmath         # noqa: F401
from vtol_reference import I_UMAX, I_AMAX, I_ALPHAT, I_ALPHAV, I_INVSIGMA, I_VD, I_CA, I_NWP_TOT, I_NWP, I_PHIOBS, I_PSIWP, I_MUOBS

D, S = 6, 12
MUTATIONS = ("tanh_no_factor", "hook_no_inv_sigma", "final_no_wp_weight", "final_no_002", "hook_no_minus_one", "no_length")


class VDual(fr.Dual):
    """fields_reference.Dual on numpy.float64 values (0 / 0 is a NaN, not an exception) with the tanh rule of dual.hpp:
    th = tanh(a.v); (th, (1.0 - th th) a.d)."""
    __slots__ = ()
    __array_ufunc__ = None           # numpy.float64 * VDual is VDual.__rmul__, not a ufunc over an object
    SQRT = staticmethod(np.sqrt)
    TANH = staticmethod(np.tanh)
    TANH_FACTOR = True

    def tanh(self):
        th = self.TANH(self.v)
        return self._new(th, (1.0 - th * th) * self.d if self.TANH_FACTOR else 1.0 * self.d)


class VDualNoFactor(VDual):
    __slots__ = ()
    TANH_FACTOR = False


if HAVE_MPMATH:
    class VDualMpf(VDual):
        __slots__ = ()
        SQRT = staticmethod(lambda x: mpmath.sqrt(x))
        TANH = staticmethod(lambda x: mpmath.tanh(x))

    class VDualMpfNoFactor(VDualMpf):
        __slots__ = ()
        TANH_FACTOR = False


class Carrier:
    """What a text needs beside the numbers: the dual class, the zero derivative part, and the decisions taken
    (margins[name] = the value the decision read)."""

    def __init__(self, cls, zero, high):
        self.cls, self.zero, self.high = cls, zero, high
        self.margins = {}

    def number_zero(self):
        z = self.zero.copy() if isinstance(self.zero, np.ndarray) else self.zero
        return self.cls(mpf(0) if self.high else F64(0.0), z)

    def note(self, name, v):
        self.margins[name] = min(self.margins.get(name, abs(v)), abs(v))


def control_t(C, P, X):
    a_max, u_max = P[I_AMAX], P[I_UMAX]
    u = [-X[9] / a_max, -X[10] / a_max, -X[11] / a_max]
    norm_u = (u[0]*u[0] + u[1]*u[1] + u[2]*u[2]).sqrt()
    C.note("norm_u-u_max", norm_u.v - u_max)
    if norm_u.v > u_max:
        u = [u[0] / norm_u*u_max, u[1] / norm_u*u_max, u[2] / norm_u*u_max]
    return u


def map_exact_t(C, P, tab, px, py, pz, want_f, want_g):
    """map_exact_t<WANT_F, WANT_G, T>: (func, [g0, g1, g2])."""
    mu = P[I_MUOBS]
    f, g0, g1, g2 = C.number_zero(), C.number_zero(), C.number_zero(), C.number_zero()
    for i, (typ, x, y, z, radx, rady, radz) in enumerate(tab):
        if typ == 0:
            hx, hy, hz = px - x, py - y, pz - z
            d = (hx*hx + hy*hy + hz*hz).sqrt()
            if want_f:
                rad = d / (hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz).sqrt()
                h = (d - rad) / mu
                f = f + (1 - h.tanh()) / 2
            if want_g:
                q = (hx*hx / radx / radx + hy*hy / rady / rady).sqrt()
                rad = d / q
                h = (d - rad) / mu
                rho2 = (radx*radx - rady*rady) / (radx*radx*rady*rady) / q / q / q
                th = h.tanh()
                g0 = g0 - hx / d*(1 - hy*hy*rho2) / mu*(1 - th*th) / 2
                g1 = g1 - hy / d*(1 + hx*hx*rho2) / mu*(1 - th*th) / 2
                g2 = g2 - 0
        elif typ == 1:
            dx, dy, dz = px - x, py - y, pz - z
            for q in (dx, dy, dz):
                C.note("box centre plane", q.v)
            thx = ((abs(dx) - radx) / mu).tanh()
            thy = ((abs(dy) - rady) / mu).tanh()
            thz = ((abs(dz) - radz) / mu).tanh()
            if want_f:
                f = f + (1 - thx)*(1 - thy)*(1 - thz) / 8
            if want_g:
                g0 = g0 - dx / abs(dx) / mu*(1 - thx*thx)*(1 - thy)*(1 - thz) / 8
                g1 = g1 - dy / abs(dy) / mu*(1 - thy*thy)*(1 - thx)*(1 - thz) / 8
                g2 = g2 - dz / abs(dz) / mu*(1 - thz*thz)*(1 - thx)*(1 - thy) / 8
    f, g0, g1, g2 = (C.number_zero() if q.v != q.v else q for q in (f, g0, g1, g2))
    phi, psi = P[I_PHIOBS], P[I_PSIWP]
    return phi*f + psi*0.0, [phi*g0 + psi*0.0, phi*g1 + psi*0.0, phi*g2 + psi*0.0]


def rhs_t(C, P, tab, X):
    vx, vy, vz, p_x, p_y, p_z, p_vx, p_vy, p_vz = X[3:12]
    a_max, ca, alphaV, Vd = P[I_AMAX], P[I_CA], P[I_ALPHAV], P[I_VD]
    u = control_t(C, P, X)
    g = map_exact_t(C, P, tab, X[0], X[1], X[2], False, True)[1]
    d = [None] * 12
    d[0], d[1], d[2] = vx, vy, vz
    d[6], d[7], d[8] = 0 - g[0], 0 - g[1], 0 - g[2]
    normV = (vx*vx + vy*vy + vz*vz).sqrt()
    C.note("normV", normV.v)
    d[3] = a_max*u[0] - ca*vx*normV
    d[4] = a_max*u[1] - ca*vy*normV
    d[5] = a_max*u[2] - ca*vz*normV
    d[9] = -p_x + ca*(p_vx*(normV + vx*vx/normV) + p_vy*(vy*vx/normV) + p_vz*(vz*vx/normV)) - alphaV*vx/normV*(normV - Vd)
    d[10] = -p_y + ca*(p_vy*(normV + vy*vy/normV) + p_vx*(vx*vy/normV) + p_vz*(vz*vy/normV)) - alphaV*vy/normV*(normV - Vd)
    d[11] = -p_z + ca*(p_vz*(normV + vz*vz/normV) + p_vx*(vx*vz/normV) + p_vy*(vy*vz/normV)) - alphaV*vz/normV*(normV - Vd)
    return d


def hamiltonian_t(C, P, tab, X):
    vx, vy, vz, p_x, p_y, p_z, p_vx, p_vy, p_vz = X[3:12]
    a_max, ca, alphaV, Vd = P[I_AMAX], P[I_CA], P[I_ALPHAV], P[I_VD]
    normV = (vx*vx + vy*vy + vz*vz).sqrt()
    u = control_t(C, P, X)
    norm_u = (u[0]*u[0] + u[1]*u[1] + u[2]*u[2]).sqrt()
    obs = map_exact_t(C, P, tab, X[0], X[1], X[2], True, False)[0]
    return (P[I_ALPHAT]*1
            + alphaV / 2*(normV - Vd)*(normV - Vd)
            + obs
            + a_max*a_max*norm_u*norm_u / 2
            + p_x*vx + p_y*vy + p_z*vz
            + (p_vx*(a_max*u[0] - ca*vx*normV) + p_vy*(a_max*u[1] - ca*vy*normV) + p_vz*(a_max*u[2] - ca*vz*normV)))


def final_row_t(P, j, mode, X, xd, mutate=()):
    dxj = X[j] - xd[j]
    if mode == FREE:
        if "final_no_wp_weight" in mutate:
            return X[j + D] - 0.02*dxj
        if "final_no_002" in mutate:
            return X[j + D] - P[I_INVSIGMA]*(P[I_NWP_TOT] - P[I_NWP])*dxj
        return X[j + D] - P[I_INVSIGMA]*(P[I_NWP_TOT] - P[I_NWP])*dxj - 0.02*dxj
    return dxj


def switching_state_t(P, j, X, Xp, xd, mutate=()):
    fs = X[j] - Xp[j]
    if "hook_no_inv_sigma" in mutate:
        return fs, X[j + D] - Xp[j + D]
    return fs, (X[j + D] - Xp[j + D]) - P[I_INVSIGMA]*(X[j] - xd[j])


# ---- the value parts against the reference's restatement -------------------------------------------------------------------------

def plain_texts(P, table, X):
    """(rhs[12], H) of the texts over T in numpy.float64, the derivative parts empty: the value parts."""
    C = Carrier(VDual, np.zeros(0), False)
    Pn = [F64(p) for p in P]
    tab = [(float(r[0]),) + tuple(F64(v) for v in r[1:7]) for r in np.asarray(table, dtype=float).reshape(-1, 7)]
    Xn = [VDual(F64(x), np.zeros(0)) for x in X]
    with np.errstate(all="ignore"):
        return np.array([q.v for q in rhs_t(C, Pn, tab, Xn)], dtype=F64), F64(hamiltonian_t(C, Pn, tab, Xn).v)


def reference_texts(P, table, X):
    """(rhs[12], H) of vtol_reference.vtol_ref on F64Kit: what the value parts above must equal bit for bit."""
    d, _, H = vr.emulate(vr.vtol_ref, P, table, X)
    return d, H


# ---- the definition ----------------------------------------------------------------------------------------------------------------

def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


def exact_jacobian_row(P, table, prob, z, N, high=False, derivs=True, mutate=(), margins=None, end_states=None):
    """One row of the batch: (J, F), J[row][col] = dF_row / dz_col (n x n: float64, or dtype object in 240 bits), F[n].  high: the
    same recurrence in 240 bits, z may then hold mpf numbers.  derivs=False: the value parts alone (the residual).  margins: a dict
    that receives the smallest |margin| of every decision; end_states: a list that receives the value parts at the end of each
    segment."""
    assert set(mutate) <= set(MUTATIONS)
    lay = Layout(prob)
    M, n = lay.M, lay.n
    assert lay.S == S and lay.D == D
    no_factor = "tanh_no_factor" in mutate
    cls = (VDualMpfNoFactor if no_factor else VDualMpf) if high else (VDualNoFactor if no_factor else VDual)
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else F64
    G = S + 1 if derivs else 0
    vec = lambda vals: np.array([num(v) for v in vals], dtype=object if high else np.float64)      # noqa: E731
    zero = vec([0.0] * G)
    C = Carrier(cls, zero, high)
    zz, Pn = [num(v) for v in z], [num(p) for p in P]
    tab = [(float(r[0]),) + tuple(num(v) for v in r[1:7]) for r in np.asarray(table, dtype=float).reshape(-1, 7)]
    xn = [[num(v) for v in row] for row in prob.xnode]
    J = np.array([[num(0.0)] * n for _ in range(n)], dtype=object if high else np.float64).reshape(n, n)
    F = [num(0.0)] * n

    jt = lambda j: zz[lay.kind[j]] if lay.kind[j] >= 0 else num(prob.time[j])                       # noqa: E731

    def nt(k):
        if lay.kind[k] >= -1:
            return jt(k)
        a, b = lay.lo[k], lay.hi[k]
        ta, tb = jt(a), jt(b)
        return ta + (k - a) * (tb - ta) / (b - a)

    def weight(j, f):
        if j == f:
            return num(1.0)
        if lay.kind[j] != -2:
            return num(0.0)
        a, b = lay.lo[j], lay.hi[j]
        q = num(j - a) / num(b - a)
        return q if f == b else (num(1.0) - q if f == a else num(0.0))

    def rk4(X, h):
        f = lambda Y: rhs_t(C, Pn, tab, Y)          # noqa: E731  (the right-hand side is autonomous)
        h2 = h / 2.0
        F1 = f(X)
        Y = [x + h2 * k for x, k in zip(X, F1)]
        F2 = f(Y)
        Y = [x + h2 * k for x, k in zip(X, F2)]
        F3 = f(Y)
        Y = [x + h * k for x, k in zip(X, F3)]
        Fs = [a + b for a, b in zip(F2, F3)]
        F4 = f(Y)
        h6 = h / 6.0
        return [x + h6 * (k1 + (k4 + 2.0 * ks)) for x, k1, k4, ks in zip(X, F1, F4, Fs)]

    with np.errstate(all="ignore"):
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
                    H = hamiltonian_t(C, Pn, tab, X)
                    put_state(lay.ft_row[0], H)
                    F[lay.ft_row[0]] = H.v
            elif derivs:
                for c in range(S):
                    mode = prob.mode_x[i][c % D]
                    if mode == FIXED:
                        if c < D:
                            J[first + D + c, first + c] = num(1.0)
                    elif not (mode == FREE and "hook_no_minus_one" in mutate):
                        J[first + c, first + c] = num(-1.0)
                if lay.ft_row[i] >= 0:                                   # kSwitchingReadsXp: -grad H(X+)
                    put_state(lay.ft_row[i], -hamiltonian_t(C, Pn, tab, X))

            # ---- the loop of Lane::integrate on duals, the step length a dual number
            t2d = cls(t2, vec([0.0] * S + [1.0]) if derivs else zero)
            t = cls(t1, zero)
            dt = (t2d - t) / N
            guard = N + 8
            while t.v < (t2 - dt.v / 2) and guard > 0:
                guard -= 1
                step = (t2d - t) if (t.v + dt.v > t2) else dt
                X = rk4(X, step)
                t = t + dt
            if end_states is not None:
                end_states.append([q.v for q in X])

            # ---- the free times the segment's length depends on
            A = lay.lo[i] if lay.kind[i] == -2 else i
            Bn = lay.hi[i + 1] if lay.kind[i + 1] == -2 else i + 1
            frees = []
            for f in (A, Bn):
                if lay.kind[f] >= 0 and "no_length" not in mutate:
                    w = weight(i + 1, f) - weight(i, f)
                    if w != 0:
                        frees.append((lay.kind[f], w))

            def emit(row, e, deriv=True):
                F[row] = e.v
                if deriv and derivs:
                    put_state(row, e)
                    for k, w in frees:
                        J[row, k] = w * e.d[S]

            # ---- the rows on the END state
            if i < M - 1:
                Xp = zz[S * (i + 1):S * (i + 2)]
                if lay.ft_row[i + 1] >= 0:
                    emit(lay.ft_row[i + 1], hamiltonian_t(C, Pn, tab, X) - hamiltonian_t(C, Pn, tab, [cls(x, zero) for x in Xp]))
                for j in range(D):
                    row = S * (i + 1) + j
                    mode = prob.mode_x[i + 1][j]
                    xdj = xn[i + 1][j]
                    if mode == FIXED:
                        emit(row, X[j] - xdj)
                        F[row + D] = Xp[j] - xdj
                    elif mode == FREE:
                        fs, fc = switching_state_t(Pn, j, X, Xp, xn[i + 1], mutate)
                        emit(row, fs)
                        emit(row + D, fc)
                    else:
                        emit(row, X[j] - Xp[j])
                        emit(row + D, X[j + D] - Xp[j + D])
            if i == M - 1:
                for j in range(D):
                    emit(D + j, final_row_t(Pn, j, prob.mode_x[M][j], X, xn[M], mutate))
                if lay.ft_row[M] >= 0:
                    emit(lay.ft_row[M], hamiltonian_t(C, Pn, tab, X) + 0.0)      # final_h_offset
    if margins is not None:
        for k, v in C.margins.items():
            margins[k] = min(margins.get(k, v), v)
    return J, (F if high else np.array(F, dtype=np.float64))


def exact_jacobian_batch(P, table, prob, Z, N, blocks=None):
    """What the call leaves: (Fjac[B][n*n] COLUMN-major, F[B][n]) in doubles.  blocks = (params[B][13 + 2], time[B][M+1],
    xnode[B][(M+1) 12]), any of them None."""
    from oracle.oracle import Problem
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    Js, Fs = [], []
    for b, z in enumerate(Z):
        Pb = P if pp is None else pp[b][:len(P)]
        pb = prob if tt is None and xx is None else Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time if tt is None else tt[b],
                                                             prob.xnode if xx is None else xx[b])
        J, F = exact_jacobian_row(Pb, table, pb, z, N)
        Js.append(np.ascontiguousarray(J.T).ravel())
        Fs.append(F)
    return np.array(Js), np.array(Fs)


def fields_segment(P, table, t1, t2, X0, N, cols=fr.ALL, stride=1, skip=0):
    """One slab of socp_fields_batch in doubles (fields_reference.fields_segment's dict) with this module's right-hand side: plain
    t and h, C columns travelling together."""
    from jacobi_reference import det_reference
    Cn = S if cols == fr.ALL else D
    first = 0 if cols == fr.ALL else D
    zero = np.zeros(Cn)
    C = Carrier(VDual, zero, False)
    Pn = [F64(p) for p in P]
    tab = [(float(r[0]),) + tuple(F64(v) for v in r[1:7]) for r in np.asarray(table, dtype=float).reshape(-1, 7)]
    X = [VDual(F64(X0[j]), np.array([1.0 if j == first + c else 0.0 for c in range(Cn)])) for j in range(S)]
    f = lambda Y: rhs_t(C, Pn, tab, Y)          # noqa: E731
    out = dict(tq=[], det=[])
    t1, t2 = F64(t1), F64(t2)
    dt = (t2 - t1) / N
    t = t1
    guard = N + 8
    k = 0
    act = t < (t2 - dt / 2) and guard > 0
    guard -= 1 if act else 0
    with np.errstate(all="ignore"):
        while act:
            h = (t2 - t) if (t + dt > t2) else dt
            h2 = h / 2.0
            F1 = f(X)
            Y = [x + h2 * q for x, q in zip(X, F1)]
            F2 = f(Y)
            Y = [x + h2 * q for x, q in zip(X, F2)]
            F3 = f(Y)
            Y = [x + h * q for x, q in zip(X, F3)]
            Fs = [a + b for a, b in zip(F2, F3)]
            F4 = f(Y)
            h6 = h / 6.0
            X = [x + h6 * (k1 + (k4 + 2.0 * ks)) for x, k1, k4, ks in zip(X, F1, F4, Fs)]
            tq = t + h
            t = t + dt
            k += 1
            act = t < (t2 - dt / 2) and guard > 0
            guard -= 1 if act else 0
            if k % stride == 0 or not act:
                Jm = np.array([[float(X[r].d[Cn - D + cc]) for cc in range(D)] for r in range(D)])
                out["tq"].append(float(tq))
                out["det"].append(det_reference(Jm, True)[0])
    out["count"] = len(out["det"])
    out["nchange"], out["tconj"] = fr.detect(out["tq"], out["det"], skip)
    out["phi"] = np.array([[float(X[r].d[c]) for c in range(Cn)] for r in range(S)], dtype=np.float64)
    return out


# ---- stages of tests/golden/vtol_flow.npz ------------------------------------------------------------------------------------------

def stage(flow, name, ca=None, alphaV=None):
    """(params[13], Problem, z*) of a stored stage, with ca / alphaV replaced when given."""
    from oracle.oracle import Problem
    mode_t = flow[name + "_mode_t"].astype(np.int32)
    M = len(mode_t) - 1
    mode_x = flow[name + "_mode_X"].astype(np.int32).reshape(M + 1, D)
    xnode = np.zeros((M + 1, S))
    xnode[:, 0:D] = flow[name + "_xd"].reshape(M + 1, D)
    P = np.array(flow[name + "_params"], dtype=np.float64)
    if ca is not None:
        P[I_CA] = ca
    if alphaV is not None:
        P[I_ALPHAV] = alphaV
    prob = Problem(D, mode_t, mode_x, np.array(flow[name + "_time"], dtype=np.float64), xnode)
    return P, prob, np.array(flow[name + "_z"], dtype=np.float64)


# ---- the figures shared by test_vtol_exact_cpu.py, golden/make_vtol_exact_golden.py and test_gpu_vtol_exact.py ----------------------

N_STEPS = 10                     # RK4 steps per segment
CA = ALPHAV = 0.05               # the stored stages have alphaV = 0 (and path_1 ca = 0): both terms are switched on
STAGES = ("path_1", "path_2")
NEWTON_SEED, NEWTON_STARTS = 20261021, 8


def newton_starts(z, factor):
    """z* + factor max(1, |z*|) xi, xi uniform in [-1, 1], NEWTON_STARTS rows from the fixed seed."""
    xi = np.random.default_rng(NEWTON_SEED).uniform(-1.0, 1.0, size=(NEWTON_STARTS, len(z)))
    return z[None, :] + factor * np.maximum(1.0, np.abs(z))[None, :] * xi


def newton_rows(P, table, prob, starts, N=N_STEPS, **opts):
    """tests/newton_reference.py's iteration (the definition of socp_newton_batch) on the restated residual and Jacobian, jac = 2:
    the arrays of newton_reference.stack."""
    import newton_reference as nr
    res = lambda y: exact_jacobian_row(P, table, prob, y, N, derivs=False)[1]     # noqa: E731
    jac = lambda y, F0: exact_jacobian_row(P, table, prob, y, N)[0]               # noqa: E731
    return nr.stack([nr.polish(res, jac, z0, dict(opts, jac=2)) for z0 in starts])


def amax(A):
    return max(abs(q) for q in np.asarray(A).ravel())


def to_double(A):
    return np.array([float(q) for q in np.asarray(A).ravel()], dtype=np.float64).reshape(np.asarray(A).shape)


def dev_of(J, Jh):
    """max |J - J240| / max |J240| of a double matrix against the 240-bit one."""
    return float(max(abs(mpf(float(a)) - b) for a, b in zip(np.asarray(J).ravel(), np.asarray(Jh).ravel())) / amax(Jh))
