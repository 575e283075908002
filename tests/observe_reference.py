"""The definition of socp_observe_batch restated in numpy (helper of test_observe_cpu.py / test_gpu_observe_batch.py, not a test).

A segment's rows are the rows socp_trace_batch keeps with stride = 1, in the trace's format [R][W] = t, X[S], u[NU], H, aux0, aux1.
The observables of a row are functions of (t, X, u), of the packed parameter block and, for vtolUAV, of the obstacle table
(7 doubles per obstacle: type, centre xyz, radii xyz): OBSERVE[model] restates every in-tree model's and the osc1d_observe plugin's,
operation by operation as include/socp_hip.h writes them, on numpy.float64 scalars -- one rounding per operation -- with the
conventions of fast_reference.F64Kit; exp is libm's (math.exp: numpy's exp is NOT), which is what exp_glibc reproduces.
The reduction is ONE model-independent function, reduce_rows, sequential in row order, so a result can be compared bit for bit:
    row 0:  ymin = ymax = y, tmin = tmax = t, I = +0.0
    later:  if y < ymin: ymin, tmin = y, t;   if y > ymax: ymax, tmax = y, t;   w = t - t_prev;  s = y + y_prev;  I = I + (0.5 w) s
nbad = the rows in which some observable is not finite."""
import math

import numpy as np

from extrema_reference import GUARD, SENT, SENT_I, greater, less, sentinel, sentinel_i, u64  # noqa: F401  (re-exported for the tests)
from fast_reference import F64Kit

F64 = np.float64
KIT = F64Kit(exp=lambda x: F64(math.exp(float(x))))
INF = F64(np.inf)


# ---- the observables ------------------------------------------------------------------------------------------------------------

def goddard_observe(P, t, X, u, table=None, K=KIT):
    """P: C, b, KD, kr, ...  ->  r, v, norm_u, drag, drag_acc, fuel_rate."""
    b, KD, kr = F64(P[1]), F64(P[2]), F64(P[3])
    r = K.sqrt(X[0]*X[0] + X[1]*X[1] + X[2]*X[2])
    v = K.sqrt(X[3]*X[3] + X[4]*X[4] + X[5]*X[5])
    E = K.exp(-kr*(r - 1))
    norm_u = K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])
    drag = KD*v*v*E
    return [r, v, norm_u, drag, drag / X[6], b*norm_u]


def box_level(px, py, pz, o):
    m = abs(px - o[1]) - o[4]
    b = abs(py - o[2]) - o[5]
    c = abs(pz - o[3]) - o[6]
    if b > m:
        m = b
    if c > m:
        m = c
    return m


def ellipsoid_level(px, py, pz, o, K=KIT):
    hx, hy, hz = px - o[1], py - o[2], pz - o[3]
    radx, rady, radz = o[4], o[5], o[6]
    d = K.sqrt(hx*hx + hy*hy + hz*hz)
    return d - d / K.sqrt(hx*hx / radx / radx + hy*hy / rady / rady + hz*hz / radz / radz)


def clearance(px, py, pz, table, box=box_level, ellipsoid=ellipsoid_level, below=less):
    """The smallest level of any obstacle, in table order under a strict comparison; +inf for an empty table."""
    cl = INF
    px, py, pz = F64(px), F64(py), F64(pz)
    for o in np.asarray(table, dtype=F64).reshape(-1, 7):
        if o[0] == 0:
            with np.errstate(all="ignore"):
                level = ellipsoid(px, py, pz, o)
        elif o[0] == 1:
            level = box(px, py, pz, o)
        else:
            continue
        if below(level, cl):
            cl = level
    return cl


def vtol_observe(P, t, X, u, table=None, K=KIT):
    """speed, norm_u, clearance."""
    return [K.sqrt(X[3]*X[3] + X[4]*X[4] + X[5]*X[5]), K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]),
            clearance(X[0], X[1], X[2], table if table is not None else np.zeros((0, 7)))]


def dint_observe(P, t, X, u, table=None, K=KIT):
    return [K.sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2])]


def covid_observe(P, t, X, u, table=None, K=KIT):
    return [u[0]]


def osc1d_observe(P, t, X, u, table=None, K=KIT):
    """tests/plugin/osc1d_observe_plugin.hip: the energy and |u|."""
    return [(X[0]*X[0] + X[1]*X[1]) / 2, abs(u[0])]


# model key -> (observe, S, NU, names)
OBSERVE = {
    "goddard": (goddard_observe, 14, 3, ["r", "v", "norm_u", "drag", "drag_acc", "fuel_rate"]),
    "vtol": (vtol_observe, 12, 3, ["speed", "norm_u", "clearance"]),
    "dint": (dint_observe, 12, 3, ["norm_u"]),
    "covid": (covid_observe, 8, 1, ["u"]),
    "osc1d_observe": (osc1d_observe, 2, 1, ["energy", "abs_u"]),
}


def observables_of_rows(model, rows, params, table=None):
    """Trace-format rows [R][W] -> (t[R], Y[R][NO])."""
    fn, S, NU, names = OBSERVE[model]
    rows = np.asarray(rows, dtype=F64)
    with np.errstate(all="ignore"):
        Y = np.array([fn(params, r[0], r[1:1 + S], r[1 + S:1 + S + NU], table) for r in rows], dtype=F64).reshape(len(rows), len(names))
    return rows[:, 0].copy(), Y


# ---- the reduction: model-independent ---------------------------------------------------------------------------------------------

def trapezoid(I, w, y, y_prev):
    return I + (F64(0.5) * w) * (y + y_prev)


def reduce_rows(t, Y, below=less, above=greater, quadrature=trapezoid):
    """t[R], Y[R][NO] -> dict(ymin, ymax, tmin, tmax, integral [NO], count, nbad): the sequential reduction, every observable on its
    own.  below / above / quadrature: the two comparisons and the quadrature step (replaced by the wrong restatements of
    test_observe_cpu.py)."""
    t, Y = np.asarray(t, dtype=F64), np.asarray(Y, dtype=F64)
    R, NO = Y.shape
    ymin, ymax = Y[0].copy(), Y[0].copy()
    tmin, tmax = np.full(NO, t[0]), np.full(NO, t[0])
    integral = np.zeros(NO)
    with np.errstate(all="ignore"):
        for k in range(1, R):
            w = t[k] - t[k - 1]
            for c in range(NO):
                y = Y[k, c]
                if below(y, ymin[c]):
                    ymin[c], tmin[c] = y, t[k]
                if above(y, ymax[c]):
                    ymax[c], tmax[c] = y, t[k]
                integral[c] = quadrature(integral[c], w, y, Y[k - 1, c])
    return dict(ymin=ymin, ymax=ymax, tmin=tmin, tmax=tmax, integral=integral, count=R,
                nbad=int(np.sum(~np.all(np.isfinite(Y), axis=1))))


def reference_observe(model, rows, params, table=None):
    """One segment: reduce_rows of the observables of its trace-format rows."""
    return reduce_rows(*observables_of_rows(model, rows, params, table))


def reference_from_trace(model, rows, count, params, table=None):
    """What trace_batch(stride = 1) returned (rows[B][M][cap][W], count[B][M], every count <= cap) -> list [b][i] of
    reference_observe; params: one packed parameter vector, or [B] of them (per-row blocks)."""
    B, M = count.shape
    assert count.max() <= rows.shape[2], "the trace's cap was too small for this comparison"
    per_row = np.ndim(params) == 2
    return [[reference_observe(model, rows[b, i, :count[b, i]], params[b] if per_row else params, table) for i in range(M)]
            for b in range(B)]


KEYS = ("ymin", "ymax", "tmin", "tmax", "integral")


def pack_observe(ref, given=(True, True, True), nbad=True):
    """What the entry points leave in guarded, sentinel-filled caller buffers: the seven WHOLE buffers (ymin, ymax, tmin, tmax,
    integral as uint64, count, nbad as int32), guard words included.  A buffer that was not passed (given = tmin, tmax, integral;
    nbad) keeps the sentinel."""
    B, M, NO = len(ref), len(ref[0]), len(ref[0][0]["ymin"])
    bufs = [np.full(B * M * NO + GUARD, SENT, dtype=np.uint64) for _ in range(5)]
    cnt, bad = sentinel_i(B * M), sentinel_i(B * M)
    on = (True, True) + tuple(given)
    for b in range(B):
        for i in range(M):
            r, T = ref[b][i], b * M + i
            for buf, key, use in zip(bufs, KEYS, on):
                if use:
                    buf[T * NO:(T + 1) * NO] = u64(r[key])
            cnt[T] = r["count"]
            if nbad:
                bad[T] = r["nbad"]
    return (*bufs, cnt, bad)
