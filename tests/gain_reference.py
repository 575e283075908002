"""The definition of socp_gain_batch (include/socp_hip.h) restated in Python, one IEEE operation per line (helper of test_gain_cpu.py
and test_gpu_gain_batch.py, not a test), on top of tests/fields_reference.py (Dual, the kits, rk4_dual and the generic-kit right-hand
sides) and the elimination of tests/tangent_reference.py.

In doubles the S columns of a segment travel together: one state whose derivative parts are numpy arrays of S doubles -- the value
parts of all columns are the same numbers and numpy's elementwise products, sums and quotients are the scalar IEEE operations.  With
high=True the same recurrence runs on 240-bit mpmath numbers (one state per column), the step sequence that of the doubles.

`mutate` names the WRONG restatements the CPU tests must catch: "no_reseed" (the derivative parts run on through a sample),
"psi_times_w" (the product taken as Psi W), "no_minus" (A_p K = +A_x), "halves_swapped" (the selector reads the other half)."""
import numpy as np

import fields_reference as fr
import tangent_reference as tr
from fields_reference import Dual, DualKit, DualMpfKit, RHS, rk4_dual, HAVE_MPMATH, mpf, mpmath   # noqa: F401

FREE = 1
MUTATIONS = ("no_reseed", "psi_times_w", "no_minus", "halves_swapped")


def step_sequence(t1, t2, N):
    """[(t, h)] of the residual's fixed-step loop, decided in doubles: t is the loop's own accumulated time."""
    t1, t2 = float(t1), float(t2)
    steps = []
    with np.errstate(all="ignore"):
        dt = (t2 - t1) / N
        t = t1
        guard = N + 8
        while t < (t2 - dt / 2) and guard > 0:
            guard -= 1
            steps.append((t, (t2 - t) if (t + dt > t2) else dt))
            t = t + dt
    return steps, t


def _seed(S, X, high, cls):
    """The state(s) (X.v, e_c): one state with array derivative parts in doubles, one state per column in 240 bits."""
    if high:
        return [[cls(X[j], mpf(1.0) if j == c else mpf(0.0)) for j in range(S)] for c in range(S)]
    return [[cls(X[j], np.array([1.0 if j == c else 0.0 for c in range(S)])) for j in range(S)]]


def _dparts(states, S, high):
    """Psi[r][c] = the derivative part of component r in column c."""
    if high:
        return np.array([[states[c][r].d for c in range(S)] for r in range(S)], dtype=object)
    return np.array([states[0][r].d for r in range(S)], dtype=np.float64)


def run_block(model, P, sw, X, steps, high=False):
    """From the value state X (doubles or 240-bit numbers) with unit seeds through `steps`: (Psi[S][S], the value state after them)."""
    S = len(X)
    cls = fr.DualMpf if high else Dual
    K = DualMpfKit() if high else DualKit()
    num = (lambda x: x if isinstance(x, mpmath.mpf) else mpf(float(x))) if high else float
    Pn, swn = [num(p) for p in P], [num(s) for s in sw]
    zero = num(0.0) if high else np.zeros(S)
    states = _seed(S, [num(x) for x in X], high, cls)
    with np.errstate(all="ignore"):
        for t, h in steps:
            states = [rk4_dual(RHS[model], K, cls, Pn, swn, num(t), Y, num(h), zero) for Y in states]
    return _dparts(states, S, high), [q.v for q in states[0]]


def gain_segment(model, P, sw, D, t1, t2, X0, N, stride, high=False, mutate=()):
    """One segment: dict(tq[Q], xq[Q][S], psi[Q][S][S], count = Q, xend).  Sample q sits at the START of step q stride; block q runs to
    the start of the next sample or to the segment's end; a segment without a step has Q = 1 and Psi_0 = I."""
    steps, _ = step_sequence(t1, t2, N)
    Q = max(1, -(-len(steps) // stride))
    out = dict(tq=[], xq=[], psi=[], count=Q)
    X = list(X0)
    carry = None                                                    # "no_reseed": the product of the blocks so far rides along
    for q in range(Q):
        blk = steps[q * stride:(q + 1) * stride]
        out["tq"].append(blk[0][0] if blk else float(t1))
        out["xq"].append([x for x in X])
        psi, X = run_block(model, P, sw, X, blk, high)
        if "no_reseed" in mutate:
            carry = psi if carry is None else matmul(psi, carry, high)
            psi = carry
        out["psi"].append(psi)
    out["xend"] = X
    return out


def matmul(A, B, high=False):
    """C[r][j] = sum_m A[r][m] B[m][j], m ascending, each product rounded, the sum sequential from the first product."""
    A, B = np.asarray(A), np.asarray(B)
    with np.errstate(all="ignore"):
        C = A[:, 0:1] * B[0:1, :]
        for m in range(1, A.shape[1]):
            C = C + A[:, m:m + 1] * B[m:m + 1, :]
    return C


def selector(mode_final, D, high=False, mutate=()):
    """E[D][S]: row j is e_{D + j} when final component j is FREE, else e_j."""
    one, zero = (mpf(1.0), mpf(0.0)) if high else (1.0, 0.0)
    E = np.array([[zero] * (2 * D) for _ in range(D)], dtype=object if high else np.float64)
    for j in range(D):
        upper = int(mode_final[j]) == FREE
        if "halves_swapped" in mutate:
            upper = not upper
        E[j, D + j if upper else j] = one
    return E


def gain_of(W, D, high=False, mutate=()):
    """(Kp[D][D] COLUMN-major, i.e. Kp[c][r] = dp_r/dx_c, info) from W = [A_x | A_p]: A_p K = -A_x."""
    Ax, Ap = W[:, :D], W[:, D:]
    rhs = Ax if "no_minus" in mutate else -Ax
    if high:
        try:
            A = mpmath.matrix(Ap.tolist())
            cols = [mpmath.lu_solve(A, mpmath.matrix([rhs[r, c] for r in range(D)])) for c in range(D)]
        except ZeroDivisionError:                                     # an exactly singular A_p (the thrust is off to the end)
            return None, 1
        return np.array([[cols[c][r] for r in range(D)] for c in range(D)], dtype=object), 0
    with np.errstate(all="ignore"):
        X, info, _ = tr.eliminate(Ap, rhs.T)
    return X, info


def sweep(segments, mode_final, D, cap=None, high=False, mutate=()):
    """The backward sweep over the segments' blocks: per segment lists wq[Q][D][S], kp[Q][D][D], info[Q]."""
    W = selector(mode_final, D, high, mutate)
    if cap is not None and any(s["count"] > cap for s in segments):
        W = np.where(W == 1.0, np.nan, W)
    out = [dict(wq=[None] * s["count"], kp=[None] * s["count"], info=[0] * s["count"]) for s in segments]
    for i in range(len(segments) - 1, -1, -1):
        for q in range(min(segments[i]["count"], cap if cap is not None else segments[i]["count"]) - 1, -1, -1):
            psi = segments[i]["psi"][q]
            W = matmul(psi, W.T, high).T if "psi_times_w" in mutate else matmul(W, psi, high)      # (Psi W^T)^T = W Psi^T: the wrong side
            out[i]["wq"][q] = W
            out[i]["kp"][q], out[i]["info"][q] = gain_of(W, D, high, mutate)
    return out


def gain_row(model, P, sw, D, timeline, mode_final, z, N, stride, cap=None, high=False, mutate=()):
    """One row of the call: per segment dict(tq, xq, psi, count, wq, kp, info)."""
    S = 2 * D
    M = len(timeline) - 1
    segs = [gain_segment(model, P, sw, D, timeline[i], timeline[i + 1], z[S * i:S * (i + 1)], N, stride, high, mutate) for i in range(M)]
    for s, w in zip(segs, sweep(segs, mode_final, D, cap, high, mutate)):
        s.update(w)
    return segs


NAMES = ("tq", "Kp", "info", "count", "Xq", "Wq", "Psi")


def pack(rows, B, M, D, cap, fill_bits, fill_int, xq=True, wq=True, psi=True):
    """What the call must leave in buffers filled with fill_bits / fill_int, in the order of NAMES: uint64 views of the doubles, int32
    info and count; None for an output whose pointer is NULL.  rows[b][i] as gain_row returns them."""
    S = 2 * D
    u = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)                        # noqa: E731
    full = lambda *shape: np.full(shape, np.uint64(fill_bits), dtype=np.uint64)                    # noqa: E731
    tq, Kp, Xq, Wq, Psi = full(B, M, cap), full(B, M, cap, D, D), full(B, M, cap, S), full(B, M, cap, D, S), full(B, M, cap, S, S)
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
                Wq[b, i, q] = u(s["wq"][q])
                Kp[b, i, q] = u(s["kp"][q])
                info[b, i, q] = s["info"][q]
    return tq, Kp, info, count, (Xq if xq else None), (Wq if wq else None), (Psi if psi else None)
