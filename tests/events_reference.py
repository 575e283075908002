"""The definition of socp_events_batch restated in numpy (helper of test_events_cpu.py / test_gpu_events_batch.py, not a test).

A watch e looks at channel chan[e] of the model minus level[e] along the fixed RK4 steps the residual takes; a sign change over
a step is an event, refined inside the step by R bracketed false-position steps, each ONE RK4 step of length th from the state
before the step.  Every operation below is one IEEE double operation in the order the reference-order kernel performs it
(integrate_events, socp_amd/csrc/segment_views.hpp), the RK4 step is the CPU oracle's (Oracle.rk4_step), and the three channel
expressions are restated from the reference's lines, so a result can be compared bit for bit."""
import numpy as np

F64 = np.float64


# ---- the models' event channels: event_fn(p, X, chan) with p the packed parameters --------------------------------------------

def goddard_event(p, X, chan):
    """goddard.cpp:135  Switch = mu1 - b*p_mass - C / mass*norm_pv,  norm_pv as at :130.  p = (C, b, KD, kr, u_max, mu1, mu2, sing)."""
    C, b, mu1 = F64(p[0]), F64(p[1]), F64(p[5])
    mass, p_vx, p_vy, p_vz, p_mass = F64(X[6]), F64(X[10]), F64(X[11]), F64(X[12]), F64(X[13])
    norm_pv = np.sqrt(p_vx*p_vx + p_vy*p_vy + p_vz*p_vz)
    return mu1 - b*p_mass - C / mass*norm_pv


def dint_event(p, X, chan):
    """doubleIntegrator.cpp:218-259 before the rescaling: |u|, u = -p_v / a_max.  p = (u_max, a_max, muT)."""
    a_max = F64(p[1])
    u0, u1, u2 = -F64(X[9]) / a_max, -F64(X[10]) / a_max, -F64(X[11]) / a_max
    return np.sqrt(u0*u0 + u1*u1 + u2*u2)


def covid_event(p, X, chan):
    """covid19.cpp:97-126, the control before its clamp (channel 0); I = X[2] (channel 1).
    p = (R0, Tinf, Tinc, N, Imax, muI, umin, umax)."""
    if chan == 1:
        return F64(X[2])
    R0, Tinf, N = F64(p[0]), F64(p[1]), F64(p[3])
    return (F64(X[5]) - F64(X[4]))*F64(X[0])*F64(X[2]) / Tinf / N * R0


def neg(v):
    return bool(v < 0.0)


# ---- one segment --------------------------------------------------------------------------------------------------------------

def reference_events(step, event, t1, t2, X, N, chan, level, R, margins=None, channels=None):
    """The loop of Lane::integrate (dt = (t2 - t1)/N, t accumulated by t += dt, last step clamped to t2 - t, no step when
    t2 <= t1 + dt/2) with the watches.  step(t, X, h) -> the state one RK4 step of length h later; event(X, chan) -> channel value.
    Returns the events in (step, e) order: dicts(k = step index, e, t, id, X = the state at the event).
    margins (a list) receives |g - level| of every watch at every step end; channels (a dict chan -> list) the channel values."""
    X = np.array(X, dtype=F64)
    t1, t2 = F64(t1), F64(t2)
    used = sorted(set(int(c) for c in chan))
    out = []
    dt = (t2 - t1) / N
    t = t1
    g0 = {c: event(X, c) for c in used}
    if channels is not None:
        for c in used:
            channels.setdefault(c, []).append(g0[c])
    guard = N + 8
    k = 0
    while t < (t2 - dt / 2) and guard > 0:
        guard -= 1
        h = (t2 - t) if (t + dt > t2) else dt
        Xk = X
        X = step(t, Xk, h)
        g1 = {c: event(X, c) for c in used}
        if channels is not None:
            for c in used:
                channels[c].append(g1[c])
        for e in range(len(chan)):
            ch, lv = int(chan[e]), F64(level[e])
            a0, a1 = g0[ch] - lv, g1[ch] - lv
            if margins is not None:
                margins.append(min(abs(a0), abs(a1)))
            if a0 == a0 and a1 == a1 and neg(a0) != neg(a1):
                a, c, ga, gc = F64(0.0), h, a0, a1
                for _ in range(R):
                    th = a + (c - a) * (ga / (ga - gc))
                    Y = step(t, Xk, th)
                    gt = event(Y, ch) - lv
                    if neg(gt) == neg(ga):
                        a, ga = th, gt
                    else:
                        c, gc = th, gt
                th = a + (c - a) * (ga / (ga - gc))
                out.append(dict(k=k, e=e, t=t + th, id=(e + 1) if neg(a0) else -(e + 1), X=step(t, Xk, th)))
        g0 = g1
        t = t + dt
        k += 1
    return out


# ---- a batch, on the CPU oracle -------------------------------------------------------------------------------------------------

EVENT_FN = {1: goddard_event, 2: dint_event, 3: covid_event}       # by oracle model id


def reference_events_batch(o, prob, Z, N, chan, levels, R, params=None, time=None, xnode=None, margins=None, channels=None):
    """Every segment of every row of Z on the oracle `o` (its RK4 step, its timeline) for the shooting problem `prob`.
    levels[B][E]; params[B][nparams + 2] / time[B][M+1] / xnode[B][M+1][2d]: per-row blocks (None: the oracle's / the problem's own).
    Returns a list [b][i] of the event lists of reference_events."""
    from oracle.oracle import Problem
    Z = np.asarray(Z, dtype=F64).reshape(-1, prob.n)
    levels = np.asarray(levels, dtype=F64).reshape(len(Z), -1)
    s, M = 2 * prob.dim, prob.M
    fn = EVENT_FN[o.m.model_id]
    own = o.params().copy()
    rows = []
    try:
        for b, z in enumerate(Z):
            if params is not None:
                o.set_params(params[b][:-2])
            p = o.params()
            pb = prob
            if time is not None or xnode is not None:
                pb = Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time if time is None else time[b],
                             prob.xnode if xnode is None else np.asarray(xnode[b]).reshape(M + 1, s))
            tl = o.timeline(pb, z)
            step = lambda t, X, h: o.rk4_step(float(t), X, float(h))        # noqa: E731
            event = lambda X, c: fn(p, X, c)                                # noqa: E731
            rows.append([reference_events(step, event, tl[i], tl[i + 1], z[s * i:s * (i + 1)], N, chan, levels[b], R, margins, channels)
                         for i in range(M)])
    finally:
        o.set_params(own)
    return rows


NAN_BITS = 0x7FF8000000000000


def pack_events(rows, cap, s, fill_bits=NAN_BITS, fill_id=0, xev=True):
    """What the entry points leave in caller buffers whose doubles held the bit pattern fill_bits and whose ints held fill_id:
    (t[B][M][cap], id[B][M][cap], count[B][M], Xev[B][M][cap][s] or None) -- the first min(count, cap) events of a segment stored,
    all counted, the rest untouched."""
    B, M = len(rows), len(rows[0])
    t = np.full((B, M, cap), np.uint64(fill_bits), dtype=np.uint64).view(F64)
    ident = np.full((B, M, cap), fill_id, dtype=np.int32)
    count = np.zeros((B, M), dtype=np.int32)
    X = np.full((B, M, cap, s), np.uint64(fill_bits), dtype=np.uint64).view(F64) if xev else None
    for b in range(B):
        for i in range(M):
            count[b, i] = len(rows[b][i])
            for k, ev in enumerate(rows[b][i][:cap]):
                t[b, i, k], ident[b, i, k] = ev["t"], ev["id"]
                if xev:
                    X[b, i, k] = ev["X"]
    return t, ident, count, X
