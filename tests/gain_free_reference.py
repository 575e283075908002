"""The definition of socp_gain_free_batch (include/socp_hip.h) restated in Python, one IEEE operation per line (helper of
test_gain_free_cpu.py and test_gpu_gain_free_batch.py, not a test), on top of tests/gain_reference.py (the selector, the product W Psi),
tests/exact_jacobian_reference.py (the layout, the Hamiltonians, the dual loop with a dual step) and the elimination of
tests/tangent_reference.py.

The S + 1 columns of a segment travel together: one state whose derivative parts are numpy arrays of S + 1 entries, entry S the LENGTH
column -- float64 arrays (the kernels must reproduce every output bit for bit) or, with high=True, arrays of 240-bit mpmath numbers:
the same recurrence, where the unknowns may be 240-bit numbers themselves.

`mutate` names the WRONG restatements the CPU tests must catch: "no_len" (the l term dropped: wtau stays 0), "w_one" (w_i taken as 1),
"len_after" (l applied after W <- W Psi), "gradh_unreseeded" (the H row from the derivative parts the last block left),
"border_sign" (the border column enters the system with the other sign), "reseed_time" (the derivative parts of t and dt re-seeded
at a sample too)."""
import numpy as np

import fields_reference as fr
import gain_reference as gr
import tangent_reference as tr
from exact_jacobian_reference import Layout, hamiltonian_on, FIXED, FREE, CONTINUOUS   # noqa: F401
from fields_reference import Dual, DualKit, DualMpfKit, RHS, rhs_on, _as_dual, HAVE_MPMATH, mpf, mpmath   # noqa: F401

MUTATIONS = ("no_len", "w_one", "len_after", "gradh_unreseeded", "border_sign", "reseed_time")


def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


class _Carrier:
    """The number type of one run: doubles, or 240-bit numbers."""

    def __init__(self, S, high):
        self.S, self.high = S, high
        self.K = DualMpfKit() if high else DualKit()
        self.cls = fr.DualMpf if high else Dual
        self.num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
        self.zero = self.vec([0.0] * (S + 1))

    def vec(self, vals):
        return np.array([self.num(v) for v in vals], dtype=object if self.high else np.float64)

    def seed(self, j):
        """The derivative parts of component j after a re-seed: e_j in the state columns, +0.0 in the length column."""
        return self.vec([1.0 if c == j else 0.0 for c in range(self.S)] + [0.0])


def timeline(prob, lay, zz, num):
    """(nt[M + 1], w[M], nt): the node times of Timeline::nt from the row's own unknowns, w_i = c(i+1, M) - c(i, M), and nt itself."""
    M = lay.M
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

    return [nt(k) for k in range(M + 1)], [weight(i + 1, M) - weight(i, M) for i in range(M)], nt


def _rk4(C, fn, Pn, sws, t, X, h):
    """exact_jacobian_reference's step: t and h dual, h F the full dual product, the right-hand side given the value of the stage time."""
    f = lambda tt, Y: [_as_dual(C.cls, q, C.zero) for q in rhs_on(fn, C.K, Pn, sws, tt, Y)]        # noqa: E731
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


def blocks_segment(model, C, Pn, sws, t1, t2, X0, N, stride, last, mutate=(), first_step=0):
    """One segment: dict(tq[Q], xq[Q][S], psi[Q][S][S], len[Q][S], count = Q, xend, gradH[S] when `last`).  first_step > 0 starts the
    loop's clock at that step with the state X0 (a tail run: one block from a sample to the segment's end is stride >= N)."""
    S, cls, fn = C.S, C.cls, RHS[model]
    out = dict(tq=[], xq=[], psi=[], len=[], count=0)
    X = [cls(C.num(x), C.seed(j)) for j, x in enumerate(X0)]
    with np.errstate(all="ignore"):
        t2d = cls(t2, C.vec([0.0] * S + [1.0]))
        t = cls(t1, C.zero)
        dt = (t2d - t) / N
        guard = [N + 8]

        def active():
            if not t.v < (t2 - dt.v / 2):
                return False
            guard[0] -= 1
            return guard[0] >= 0

        act = active()
        for _ in range(first_step):                                    # the clock alone: t accumulates as the loop accumulates it
            t = t + dt
            act = active()
        go = True
        while go:
            out["tq"].append(t.v)
            out["xq"].append([x.v for x in X])
            X = [cls(x.v, C.seed(j)) for j, x in enumerate(X)]
            if "reseed_time" in mutate:
                t, dt = cls(t.v, C.zero), cls(dt.v, C.zero)
            left = stride
            while act and left > 0:
                step = (t2d - t) if (t.v + dt.v > t2) else dt
                X = _rk4(C, fn, Pn, sws, t, X, step)
                t = t + dt
                act = active()
                left -= 1
            out["psi"].append(np.array([x.d[:S] for x in X], dtype=object if C.high else np.float64))
            out["len"].append(np.array([x.d[S] for x in X], dtype=object if C.high else np.float64))
            out["count"] += 1
            go = act
        out["xend"] = [x.v for x in X]
        if last:
            if "gradh_unreseeded" not in mutate:
                X = [cls(x.v, C.seed(j)) for j, x in enumerate(X)]
            H = hamiltonian_on(model, C.K, Pn, sws, t2, X)
            out["gradH"] = np.array(H.d[:S], dtype=object if C.high else np.float64)
            out["H"] = H.v
    return out


def solve(W, wt, D, high=False, mutate=()):
    """(Ke[D][D + 1], info): [A_p | wtau] [K_p; k_t] = -A_x.  Ke[c] = (dp_0/dx_c .. dp_{D-1}/dx_c, dt_f/dx_c)."""
    border = -wt if "border_sign" in mutate else wt
    A = np.hstack([W[:, D:], border[:, None]])
    rhs = -W[:, :D]
    if high:
        try:
            Am = mpmath.matrix(A.tolist())
            cols = [mpmath.lu_solve(Am, mpmath.matrix([rhs[r, c] for r in range(D + 1)])) for c in range(D)]
        except (ZeroDivisionError, TypeError):                        # exactly singular (the thrust is off to the end): a zero pivot, or
            return None, 1                                            # mpmath's pivot search finding no row at all in a zero column
        return np.array([[cols[c][r] for r in range(D + 1)] for c in range(D)], dtype=object), 0
    with np.errstate(all="ignore"):
        X, info, _ = tr.eliminate(A, rhs.T)
    return X, info


def dot_len(W, l):
    """sum_m W[r][m] l[m] for every row r: m ascending, each product rounded, the sum sequential from the first product."""
    with np.errstate(all="ignore"):
        s = W[:, 0] * l[0]
        for m in range(1, W.shape[1]):
            s = s + W[:, m] * l[m]
    return s


def sweep(segments, weights, mode_final, D, cap=None, high=False, mutate=()):
    """The bordered backward sweep over the segments' blocks: per segment lists wq[Q][D + 1][S + 1], ke[Q][D][D + 1], info[Q]."""
    num = (lambda x: mpf(x)) if high else float
    W = np.vstack([gr.selector(mode_final, D, high), segments[-1]["gradH"][None, :]])
    if cap is not None and any(s["count"] > cap for s in segments):
        W = np.where(W == 1.0, np.nan, W)
        W[D, :] = np.nan
    wt = np.array([num(0.0)] * (D + 1), dtype=object if high else np.float64)
    out = [dict(wq=[None] * s["count"], ke=[None] * s["count"], info=[0] * s["count"]) for s in segments]
    for i in range(len(segments) - 1, -1, -1):
        wi = num(1.0) if "w_one" in mutate else weights[i]
        for q in range(min(segments[i]["count"], cap if cap is not None else segments[i]["count"]) - 1, -1, -1):
            psi, l = segments[i]["psi"][q], segments[i]["len"][q]
            with np.errstate(all="ignore"):
                if "len_after" in mutate:
                    W = gr.matmul(W, psi, high)
                if wi != 0 and "no_len" not in mutate:
                    wt = wt + dot_len(W, l) * wi                       # the array first: mpmath would take it for a matrix
                if "len_after" not in mutate:
                    W = gr.matmul(W, psi, high)
            out[i]["wq"][q] = np.hstack([W, wt[:, None]])
            out[i]["ke"][q], out[i]["info"][q] = solve(W, wt, D, high, mutate)
    return out


def gain_free_row(model, P, sw, prob, z, N, stride, cap=None, high=False, mutate=()):
    """One row of the call: per segment dict(tq, xq, psi, len, count, wq, ke, info); the last one holds gradH and H too."""
    assert set(mutate) <= set(MUTATIONS)
    lay = Layout(prob)
    M, S, D = lay.M, lay.S, lay.D
    C = _Carrier(S, high)
    zz, Pn = [C.num(v) for v in z], [C.num(p) for p in P]
    nts, weights, nt = timeline(prob, lay, zz, C.num)
    sws = [nt(node) if node >= 0 else C.num(dflt) for node, dflt in zip(lay.sw_node, sw)]
    segs = [blocks_segment(model, C, Pn, sws, nts[i], nts[i + 1], zz[S * i:S * (i + 1)], N, stride, i == M - 1, mutate) for i in range(M)]
    for s, w in zip(segs, sweep(segs, weights, prob.mode_x[M], D, cap, high, mutate)):
        s.update(w)
    return segs


NAMES = ("tq", "Ke", "info", "count", "Xq", "Wq", "Psi", "Len")


def pack(rows, B, M, D, cap, fill_bits, fill_int, xq=True, wq=True, psi=True, length=True):
    """What the call must leave in buffers filled with fill_bits / fill_int, in the order of NAMES: uint64 views of the doubles, int32
    info and count; None for an output whose pointer is NULL.  rows[b][i] as gain_free_row returns them."""
    S = 2 * D
    u = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)                        # noqa: E731
    full = lambda *shape: np.full(shape, np.uint64(fill_bits), dtype=np.uint64)                    # noqa: E731
    tq, Ke, Xq, Wq = full(B, M, cap), full(B, M, cap, D, D + 1), full(B, M, cap, S), full(B, M, cap, D + 1, S + 1)
    Psi, Len = full(B, M, cap, S, S), full(B, M, cap, S)
    info = np.full((B, M, cap), fill_int, dtype=np.int32)
    count = np.full((B, M), fill_int, dtype=np.int32)
    for b in range(B):
        for i in range(M):
            s = rows[b][i]
            count[b, i] = s["count"]
            for q in range(min(s["count"], cap)):
                tq[b, i, q] = u([s["tq"][q]])[0]
                Xq[b, i, q] = u(s["xq"][q])
                Psi[b, i, q] = u(s["psi"][q])
                Len[b, i, q] = u(s["len"][q])
                Wq[b, i, q] = u(s["wq"][q])
                Ke[b, i, q] = u(s["ke"][q])
                info[b, i, q] = s["info"][q]
    return tq, Ke, info, count, (Xq if xq else None), (Wq if wq else None), (Psi if psi else None), (Len if length else None)
