"""The definition of socp_sensitivity_batch (include/socp_hip.h) restated in Python, one IEEE operation per line (helper of
test_sensitivity_cpu.py and test_gpu_sensitivity_batch.py, not a test), on top of tests/fields_reference.py (Dual, the kits, rk4_dual
and the generic-kit right-hand sides), tests/exact_jacobian_reference.py (the Hamiltonians, the layout, J itself) and the elimination
of tests/tangent_reference.py.  The Python kit is duck-typed: a parameter block of dual numbers goes through the same model texts, a
dual x dual product taking the full rule with its zero terms computed.

The directions of one kind travel together: one state whose derivative parts are numpy arrays with an entry per direction -- the
value parts of all lanes are the same numbers and numpy's elementwise products, sums and quotients are the scalar IEEE operations.
Two carriers: Python floats (the kernel must reproduce every output bit for bit) and, with high=True, 240-bit mpmath numbers (arrays
of dtype object), where z, the parameters, the times and the node states may be 240-bit numbers themselves.

`mutate` names the WRONG restatements the CPU tests must catch: "wrong_slot" (the seed placed on the next slot of the block),
"plain_in_hamiltonian" (the parameter kept plain inside hamiltonian_t / switching_fn_t), "no_ci" (the weight c(i, f) dropped from w),
"one_minus_one" (the second -1.0 of a FIXED interior component missing), "no_length" (a TIME direction stores nothing)."""
import numpy as np

import exact_jacobian_reference as ej
import fields_reference as fr
import tangent_reference as tr
from exact_jacobian_reference import Layout, hamiltonian_on, switching_on, FIXED, FREE, HAVE_MPMATH, mpf, mpmath   # noqa: F401
from fields_reference import Dual, DualKit, DualMpfKit, RHS, rhs_on, _as_dual
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE, F64

MUTATIONS = ("wrong_slot", "plain_in_hamiltonian", "no_ci", "one_minus_one", "no_length")


class Setting:
    """What a row reads beside z, duck-typed like oracle.Problem: entries may be doubles or 240-bit numbers."""

    def __init__(self, prob, time=None, xnode=None):
        self.dim, self.M, self.n = prob.dim, prob.M, prob.n
        self.mode_t, self.mode_x = prob.mode_t, prob.mode_x
        self.time = list(prob.time) if time is None else list(time)
        self.xnode = [list(r) for r in (prob.xnode if xnode is None else xnode)]


def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


def _rk4_dual_step(fn, K, cls, P, sws, t, X, h, zero):
    """exact_jacobian_reference's step: Lane::rk4's reference-order arm with a DUAL step, every h F the full dual x dual rule."""
    f = lambda tt, Y: [_as_dual(cls, q, zero) for q in rhs_on(fn, K, P, sws, tt, Y)]          # noqa: E731
    h2 = h / 2.0
    th = t + h / 2.0
    F1 = f(t.v, X)
    Y = [x + h2 * k for x, k in zip(X, F1)]
    F2 = f(th.v, Y)
    Y = [x + h2 * k for x, k in zip(X, F2)]
    F3 = f(th.v, Y)
    Y = [x + h * k for x, k in zip(X, F3)]
    Fs = [a + b for a, b in zip(F2, F3)]
    te = t + h
    F4 = f(te.v, Y)
    h6 = h / 6.0
    return [x + h6 * (k1 + (k4 + 2.0 * ks)) for x, k1, k4, ks in zip(X, F1, F4, Fs)]


def sensitivity_g(model, P, sw, prob, z, N, dirs, high=False, mutate=()):
    """G[K][n] = dF/dtheta_k of one row (float64, or dtype object in 240 bits): step 2 of the definition."""
    assert set(mutate) <= set(MUTATIONS)
    fn, lay = RHS[model], Layout(prob)
    M, S, D, n = lay.M, lay.S, lay.D, lay.n
    K = DualMpfKit() if high else DualKit()
    cls = fr.DualMpf if high else Dual
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
    vec = lambda vals: np.array([num(v) for v in vals], dtype=object if high else np.float64)      # noqa: E731
    zz, Pn = [num(v) for v in z], [num(p) for p in P]
    nparams = len(Pn)
    G = np.array([[num(0.0)] * n for _ in dirs], dtype=object if high else np.float64).reshape(len(dirs), n)

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

    def end_rows(i, Pv, t2, X, emit):
        """The rows on the END state of segment i: emit(row, derivative part)."""
        if i < M - 1:
            Xp = zz[S * (i + 1):S * (i + 2)]
            if lay.ft_row[i + 1] >= 0:
                zero = np.array([num(0.0)] * len(X[0].d), dtype=X[0].d.dtype)
                emit(lay.ft_row[i + 1], switching_on(model, K, Pv, sws, t2, X, [cls(x, zero.copy()) for x in Xp]).d)
            for j in range(D):
                row = S * (i + 1) + j
                emit(row, X[j].d)
                if prob.mode_x[i + 1][j] != FIXED:
                    emit(row + D, X[j + D].d)
        if i == M - 1:
            for j in range(D):
                emit(D + j, X[j + D].d if prob.mode_x[M][j] == FREE else X[j].d)
            if lay.ft_row[M] >= 0:
                emit(lay.ft_row[M], hamiltonian_on(model, K, Pv, sws, t2, X).d)

    # ---- SOCP_DIR_PARAM: the lanes of one (row, segment) are the entries of the derivative arrays
    lanes = [(k, index) for k, (kind, index) in enumerate(dirs) if kind == DIR_PARAM]
    if lanes:
        assert all(0 <= q < nparams for _, q in lanes), "sw0 / sw1 are refused"
        seeds = [(q + 1) % nparams if "wrong_slot" in mutate else q for _, q in lanes]
        zero = vec([0.0] * len(lanes))
        Pd = [cls(Pn[q], vec([1.0 if s == q else 0.0 for s in seeds])) for q in range(nparams)]
        Ph = Pn if "plain_in_hamiltonian" in mutate else Pd

        def store(row, d):
            for c, (k, _) in enumerate(lanes):
                G[k, row] = d[c]

        for i in range(M):
            t1, t2 = nt(i), nt(i + 1)
            X = [cls(zz[S * i + j], zero.copy()) for j in range(S)]
            if i == 0 and lay.ft_row[0] >= 0:
                H = hamiltonian_on(model, K, Ph, sws, t1, X)
                store(lay.ft_row[0], H.d if isinstance(H, Dual) else zero)
            with np.errstate(all="ignore"):
                dt = (t2 - t1) / N
                t = t1
                guard = N + 8
                while t < (t2 - dt / 2) and guard > 0:
                    guard -= 1
                    h = (t2 - t) if (t + dt > t2) else dt
                    X = fr.rk4_dual(fn, K, cls, Pd, sws, t, X, h, zero)
                    t = t + dt
                end_rows(i, Ph, t2, X, store)

    # ---- SOCP_DIR_TIME on a FIXED node: the LENGTH column of the exact Jacobian, weighted
    lanes = [(k, index) for k, (kind, index) in enumerate(dirs) if kind == DIR_TIME and lay.kind[index] == -1]
    if lanes and "no_length" not in mutate:
        zero, one = vec([0.0]), vec([1.0])
        for i in range(M):
            ws = [(k, weight(i + 1, f) - (num(0.0) if "no_ci" in mutate else weight(i, f))) for k, f in lanes]
            ws = [(k, w) for k, w in ws if w != 0]
            if not ws:
                continue
            t1, t2 = nt(i), nt(i + 1)
            X = [cls(zz[S * i + j], zero.copy()) for j in range(S)]
            with np.errstate(all="ignore"):
                t2d = cls(t2, one.copy())
                t = cls(t1, zero.copy())
                dt = (t2d - t) / N
                guard = N + 8
                while t.v < (t2 - dt.v / 2) and guard > 0:
                    guard -= 1
                    step = (t2d - t) if (t.v + dt.v > t2) else dt
                    X = _rk4_dual_step(fn, K, cls, Pn, sws, t, X, step, zero)
                    t = t + dt

                def store_w(row, d):
                    for k, w in ws:
                        G[k, row] = w * d[0]

                end_rows(i, Pn, t2, X, store_w)

    # ---- SOCP_DIR_XNODE: -1.0 at every row that reads xd[j][c]
    for k, (kind, index) in enumerate(dirs):
        if kind != DIR_XNODE:
            continue
        j, c = divmod(index, S)
        assert c < D
        if j == 0:
            if prob.mode_x[0][c] != FREE:
                G[k, c] = num(-1.0)
        elif j == M:
            if prob.mode_x[M][c] != FREE:
                G[k, D + c] = num(-1.0)
        elif prob.mode_x[j][c] == FIXED:
            G[k, S * j + c] = num(-1.0)
            if "one_minus_one" not in mutate:
                G[k, S * j + D + c] = num(-1.0)
    return G


def sensitivity_row(model, P, sw, prob, z, N, dirs):
    """One row of the call in doubles: dict(dz[K][n], info, g[K][n], J[n][n])."""
    J, _ = ej.exact_jacobian_row(model, P, sw, prob, z, N)
    G = sensitivity_g(model, P, sw, prob, z, N, dirs)
    with np.errstate(all="ignore"):
        dz, info, _ = tr.eliminate(J, -G)
    return dict(dz=dz, info=info, g=G, J=J)


_ROWS = {}


def sensitivity_batch(model, P, sw, prob, Z, N, dirs, blocks=None):
    """What the call leaves: dict(dz[B][K][n], info[B], g[B][K][n]) in doubles.  blocks = (params[B][nparams + 2], time[B][M+1],
    xnode[B][(M+1) 2d]), any of them None: row b's own parameters (then two switching times), times and node states.  A row's result
    depends on the row and its blocks alone, so equal rows are computed once."""
    from oracle.oracle import Problem
    pp, tt, xx = blocks if blocks is not None else (None, None, None)
    dirs = [(int(a), int(b)) for a, b in dirs]
    out = dict(dz=[], info=[], g=[])
    for b, z in enumerate(np.asarray(Z, dtype=F64).reshape(-1, prob.n)):
        Pb = [float(p) for p in (P if pp is None else pp[b][:len(P)])]
        swb = tuple(float(s) for s in (sw if pp is None else pp[b][len(P):len(P) + 2]))
        pb = prob if tt is None and xx is None else Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time if tt is None else tt[b],
                                                             prob.xnode if xx is None else np.asarray(xx[b]).reshape(prob.M + 1, 2 * prob.dim))
        key = (model, N, tuple(Pb), swb, z.tobytes(), np.asarray(pb.time, dtype=F64).tobytes(), np.asarray(pb.xnode, dtype=F64).tobytes(),
               np.asarray(prob.mode_t).tobytes(), np.asarray(prob.mode_x).tobytes(), tuple(dirs))
        if key not in _ROWS:
            _ROWS[key] = sensitivity_row(model, Pb, swb, pb, z, N, dirs)
        r = _ROWS[key]
        out["dz"].append(r["dz"])
        out["info"].append(r["info"])
        out["g"].append(r["g"])
    return dict(dz=np.array(out["dz"], dtype=F64), info=np.array(out["info"], dtype=np.int32), g=np.array(out["g"], dtype=F64))


# ---- the 240-bit residual as a function of one moved entry (the central differences of test_sensitivity_cpu.py) ------------------

def residual_high(model, P, sw, prob, z, N, move=None):
    """F in 240 bits with theta + delta in place of ONE entry: move = (kind, index, delta), delta a 240-bit number."""
    Pn = [mpf(float(p)) for p in P]
    time = [mpf(float(t)) for t in prob.time]
    xnode = [[mpf(float(v)) for v in row] for row in prob.xnode]
    if move is not None:
        kind, index, delta = move
        if kind == DIR_PARAM:
            Pn[index] = Pn[index] + delta
        elif kind == DIR_TIME:
            time[index] = time[index] + delta
        else:
            j, c = divmod(index, 2 * prob.dim)
            xnode[j][c] = xnode[j][c] + delta
    return ej.exact_jacobian_row(model, Pn, sw, Setting(prob, time, xnode), [mpf(float(v)) for v in z], N, high=True, derivs=False)[1]


def theta_of(P, prob, kind, index):
    """The entry a direction addresses, as a double."""
    if kind == DIR_PARAM:
        return float(P[index])
    if kind == DIR_TIME:
        return float(prob.time[index])
    j, c = divmod(index, 2 * prob.dim)
    return float(prob.xnode[j][c])
