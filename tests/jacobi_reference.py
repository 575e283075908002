"""The definition of socp_jacobi_batch (include/socp_hip.h) restated in numpy, one IEEE operation per line, on a callable
step(t, X, h) -> X that takes ONE fixed RK4 step: Oracle.rk4_step for the in-tree models, rk4_of(rhs) -- RK4 in the association
order of odeTools.cpp:89-98 -- for the example plugins, whose right-hand sides are restated here too.
Python floats are IEEE doubles and every expression below is a single rounding, so the reference-order flavour of the kernel must
reproduce every output bit for bit."""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16


def fd_eps(epsfcn):
    return math.sqrt(epsfcn if epsfcn > DBL_EPSILON else DBL_EPSILON)


def fd_step(x, eps):
    """MINPACK's fdjac1 step."""
    h = eps * abs(x)
    return eps if h == 0.0 else h


def det_reference(J, swap_sign=True):
    """(det, swaps) of a D x D matrix by the fixed sequence of the header: Gaussian elimination with partial pivoting.
    swap_sign=False is the corrupted restatement the tests must reject."""
    a = [[float(v) for v in row] for row in np.asarray(J, dtype=np.float64)]
    D = len(a)
    if not all(math.isfinite(v) for row in a for v in row):
        return float("nan"), 0
    det = 0.0
    swaps = 0
    for k in range(D):
        p = k
        best = abs(a[k][k])
        for r in range(k + 1, D):
            if abs(a[r][k]) > best:
                best = abs(a[r][k])
                p = r
        if p != k:
            for c in range(k, D):
                a[k][c], a[p][c] = a[p][c], a[k][c]
            swaps += 1
        v = a[k][k]
        if v == 0.0:
            return 0.0, swaps
        det = v if k == 0 else det * v
        for r in range(k + 1, D):
            l = a[r][k] / v
            for c in range(k + 1, D):
                prod = l * a[k][c]
                a[r][c] = a[r][c] - prod
    if swap_sign and swaps % 2 == 1:
        det = -det
    return det, swaps


def jacobi_segment(step, D, t1, t2, X0, N, eps, stride=1, skip=0, swap_sign=True, use_skip=True):
    """One slab: dict(tq, det, swaps: one entry per sample; count, nchange, tconj, jend[D][D]).  use_skip=False is the corrupted
    restatement that ignores skip."""
    X0 = np.array(X0, dtype=np.float64)
    cols = [X0.copy()]
    hs = [1.0]
    for c in range(1, D + 1):
        h = fd_step(float(X0[D + c - 1]), eps)
        Xc = X0.copy()
        Xc[D + c - 1] = Xc[D + c - 1] + h
        cols.append(Xc)
        hs.append(h)
    out = dict(tq=[], det=[], swaps=[], nchange=0, tconj=float("nan"), jend=np.zeros((D, D)))
    dt = (t2 - t1) / N
    t = t1
    guard = N + 8
    k = 0
    lo = skip if use_skip else 0
    act = t < (t2 - dt / 2) and guard > 0
    guard -= 1 if act else 0
    while act:
        h_step = (t2 - t) if (t + dt > t2) else dt
        cols = [np.asarray(step(t, X, h_step), dtype=np.float64) for X in cols]
        tq = t + h_step
        t = t + dt
        k += 1
        act = t < (t2 - dt / 2) and guard > 0
        guard -= 1 if act else 0
        if k % stride == 0 or not act:
            J = np.empty((D, D))
            for c in range(1, D + 1):
                for r in range(D):
                    diff = float(cols[c][r]) - float(cols[0][r])
                    J[r, c - 1] = diff / hs[c]
            d1, sw = det_reference(J, swap_sign)
            j = len(out["det"])
            if j >= 1 and j - 1 >= lo:
                d0, t0 = out["det"][j - 1], out["tq"][j - 1]
                if d0 == d0 and d1 == d1 and (d0 < 0.0) != (d1 < 0.0):
                    if out["nchange"] == 0:
                        den = d0 - d1
                        q = d0 / den
                        span = tq - t0
                        out["tconj"] = t0 + span * q
                    out["nchange"] += 1
            out["tq"].append(tq)
            out["det"].append(d1)
            out["swaps"].append(sw)
            out["jend"] = J
    out["count"] = len(out["det"])
    return out


def pack(slabs, B, M, D, cap, fill_bits, fill_int, jend=True):
    """What the call must leave in buffers filled with fill_bits / fill_int: (tq[B][M][cap], det[B][M][cap]) as uint64 views,
    count[B][M], nchange[B][M], tconj[B][M] (uint64), Jend[B][M][D][D] (uint64; None with jend=False).  slabs[b][i]."""
    tq = np.full((B, M, cap), np.uint64(fill_bits), dtype=np.uint64)
    det = tq.copy()
    count = np.full((B, M), fill_int, dtype=np.int32)
    nchange = count.copy()
    tconj = np.full((B, M), np.uint64(fill_bits), dtype=np.uint64)
    J = np.full((B, M, D, D), np.uint64(fill_bits), dtype=np.uint64) if jend else None
    for b in range(B):
        for i in range(M):
            s = slabs[b][i]
            k = min(s["count"], cap)
            tq[b, i, :k] = np.array(s["tq"][:k], dtype=np.float64).view(np.uint64)
            det[b, i, :k] = np.array(s["det"][:k], dtype=np.float64).view(np.uint64)
            count[b, i], nchange[b, i] = s["count"], s["nchange"]
            tconj[b, i] = np.array([s["tconj"]], dtype=np.float64).view(np.uint64)[0]
            if jend:
                J[b, i] = np.ascontiguousarray(s["jend"], dtype=np.float64).view(np.uint64)
    return tq, det, count, nchange, tconj, J


# ---- RK4 on a right-hand side, odeTools.cpp:89-98 in its association order (Lane::rk4, reference order) ---------------------

def rk4_of(rhs):
    def step(t, X, h):
        X = np.asarray(X, dtype=np.float64)
        h2 = h / 2.0
        th = t + h / 2.0
        F1 = rhs(t, X)
        Y = X + h2 * F1
        F2 = rhs(th, Y)
        Y = X + h2 * F2
        F3 = rhs(th, Y)
        Y = X + h * F3
        Fs = F2 + F3
        F4 = rhs(t + h, Y)
        h6 = h / 6.0
        return X + h6 * (F1 + (F4 + 2.0 * Fs))
    return step


def osc1d_rhs(w):
    """tests/plugin/osc1d_plugin.hip: x' = -p, p' = w x."""
    return lambda t, X: np.array([-X[1], w * X[0]])


def lqr1d_rhs(g):
    """tests/plugin/lqr1d_plugin.hip: x' = v, v' = -g p_v, p_x' = 0, p_v' = -p_x."""
    return lambda t, X: np.array([X[1], -g * X[3], 0.0, -X[2]])
