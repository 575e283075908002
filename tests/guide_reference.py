"""The definition of socp_guide_batch (include/socp_hip.h) restated in Python, one IEEE operation per line (helper of
test_guide_cpu.py and test_gpu_guide_batch.py, not a test), on top of tests/fields_reference.py (the generic-kit right-hand sides and
the RK4 step in the residual's association order, flown on numbers whose derivative part is a plain zero: the value parts are the
residual's bits, as the Xq of tests/gain_reference.py are), tests/gain_reference.py and tests/gain_free_reference.py (the tables,
the timeline) and tests/exact_jacobian_reference.py (the layout, the Hamiltonians).

One call flies ONE case: the nominal row z, its tables, one deviation dx0[d].  Doubles (the reference-order kernel must reproduce
every output bit for bit) or, with high=True, 240-bit mpmath numbers: the same recurrence, where the tables may be 240-bit themselves.

`mutate` names the WRONG restatements the CPU tests must catch: "dx_sign" (dx = x_nom - x), "kg_transposed" (the d x d block of Kg
read with rows and columns exchanged), "increment" (the correction added to the flowing costate instead of the nominal one),
"ignore_info" (a correction applied where info != 0), "xnom_neighbour" (x_nom taken from the neighbouring sample), "no_retime" (t_f
not re-timed), "clock_restart" (the re-timed clock restarted at t1')."""
import math

import numpy as np

import fields_reference as fr
import gain_free_reference as gf
from exact_jacobian_reference import Layout, hamiltonian_on, FREE
from fields_reference import HAVE_MPMATH, mpf, mpmath   # noqa: F401

MUTATIONS = ("dx_sign", "kg_transposed", "increment", "ignore_info", "xnom_neighbour", "no_retime", "clock_restart")


def _div(a, b):
    """a / b as IEEE has it: Python raises on a zero divisor where the kernel gets an infinity or a NaN."""
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


class DualIEEE(fr.Dual):
    """fields_reference.Dual on doubles with IEEE's answers where Python raises (a zero divisor, exp overflowing, the root of a negative
    number): a dispersed flight may leave the range of the doubles, and the kernel flies on."""
    __slots__ = ()
    SQRT = staticmethod(_sqrt)
    EXP = staticmethod(_exp)

    def __truediv__(self, o):
        if isinstance(o, fr.Dual):
            q = _div(self.v, o.v)
            m = q * o.d
            return self._new(q, _div(self.d - m, o.v))
        return self._new(_div(self.v, o), _div(self.d, o))

    def __rtruediv__(self, c):
        q = _div(c, self.v)
        m = q * self.d
        return self._new(q, _div(-m, self.v))


def _is_high(x):
    return HAVE_MPMATH and isinstance(x, mpmath.mpf)


def tables_of(segs, free):
    """The call's tables of one row from the segments gain_reference.gain_row / gain_free_reference.gain_free_row return:
    per segment dict(xq[Q][S], kg[Q][c][r], info[Q], count).  kg[q][c] is column c: (dp_0/dx_c .. dp_{d-1}/dx_c[, dt_f/dx_c])."""
    return [dict(xq=s["xq"], kg=s["ke" if free else "kp"], info=list(s["info"]), count=s["count"]) for s in segs]


def guide_case(model, P, sw, prob, z, N, stride, tables, dx0, every, cap=None, high=False, mutate=(), stop_at=None):
    """dict(xf[S], miss[d or d + 1], nupd, nskip, tf, dxmax, xs[M][Q] (None where the sample has no table slot), samples).
    stop_at: the row-global sample index from which on no correction is applied (the costate left flowing from that sample) -- what a
    table with info forced nonzero from that sample on must equal."""
    assert set(mutate) <= set(MUTATIONS)
    lay = Layout(prob)
    M, S, D, n = lay.M, lay.S, lay.D, lay.n
    free = int(prob.mode_t[M]) == FREE
    cls = fr.DualMpf if high else DualIEEE
    K = fr.DualMpfKit() if high else fr.DualKit()
    num = (lambda x: x if _is_high(x) else mpf(float(x))) if high else float
    # the clock: with every time FIXED the step sequence is that of the doubles in 240 bits too (the convention of gain_reference.py,
    # whose tables the flight reads); with a FREE final time it is formed in the carrier (gain_free_reference.py's)
    tnum = num if free else float
    zero = num(0.0)
    fn = fr.RHS[model]
    zz, Pn = [num(v) for v in z], [num(p) for p in P]
    tfc = [zz[n - 1] if free else None]

    def times(i):
        z2 = list(zz)
        if free:
            z2[n - 1] = tfc[0]
        nts, _, nt = gf.timeline(prob, lay, z2, tnum)
        sws = [num(nt(node)) if node >= 0 else num(dflt) for node, dflt in zip(lay.sw_node, sw)]
        return nts[i], nts[i + 1], sws

    with np.errstate(all="ignore"):
        X = [zz[j] + num(dx0[j]) for j in range(D)] + [zz[D + j] for j in range(D)]
        nupd = nskip = g = 0
        dmax = zero
        xs = []
        t2, sws = None, None
        for i in range(M):
            t1, t2, sws = times(i)
            dt = (t2 - t1) / N
            t = t1
            k = 0
            tab = tables[i]
            nq = tab["count"] if cap is None else min(tab["count"], cap)
            act = bool(t < (t2 - dt / 2)) and k < N + 8
            q = 0
            xs.append([])
            go = True
            while go:
                has = q < nq
                due = every > 0 and g % every == 0
                look = due and has
                ok = look and (tab["info"][q] == 0 or "ignore_info" in mutate)
                apply = ok and (stop_at is None or g < stop_at)
                g += 1
                if due and not apply:
                    nskip += 1
                if apply:
                    nupd += 1
                if look:
                    qn = q
                    if "xnom_neighbour" in mutate:
                        qn = q + 1 if q + 1 < nq else q - 1
                    xq = [num(v) for v in tab["xq"][qn]]
                    dx = [(xq[c] - X[c]) if "dx_sign" in mutate else (X[c] - xq[c]) for c in range(D)]
                    for c in range(D):
                        a = abs(dx[c])
                        if a > dmax:
                            dmax = a
                    if apply:
                        kg = tab["kg"][q]
                        if kg is None:                                   # a singular sample forced through ("ignore_info" in 240 bits)
                            kg = [[num(float("nan"))] * (D + 1) for _ in range(D)]
                        ent = (lambda c, r: num(kg[r][c])) if "kg_transposed" in mutate else (lambda c, r: num(kg[c][r]))
                        for r in range(D):
                            s = ent(0, r) * dx[0]
                            for c in range(1, D):
                                s = s + ent(c, r) * dx[c]
                            X[D + r] = (X[D + r] + s) if "increment" in mutate else (xq[D + r] + s)
                        if free:
                            s = num(kg[0][D]) * dx[0]
                            for c in range(1, D):
                                s = s + num(kg[c][D]) * dx[c]
                            tfn = zz[n - 1] + s
                            if tfn != tfc[0] and "no_retime" not in mutate:
                                tfc[0] = tfn
                                t1, t2, sws = times(i)
                                dt = (t2 - t1) / N
                                t = t1 if "clock_restart" in mutate else t1 + tnum(float(k)) * dt
                                act = bool(t < (t2 - dt / 2)) and k < N + 8
                xs[i].append(list(X) if has else None)
                left = stride
                while act and left > 0:
                    h = (t2 - t) if (t + dt > t2) else dt
                    Y = fr.rk4_dual(fn, K, cls, Pn, sws, num(t), [cls(x, zero) for x in X], num(h), zero)
                    X = [y.v for y in Y]
                    t = t + dt
                    k += 1
                    act = bool(t < (t2 - dt / 2)) and k < N + 8
                    left -= 1
                q += 1
                go = act
        xd = prob.xnode[M]
        miss = [X[D + j] if int(prob.mode_x[M][j]) == FREE else X[j] - num(xd[j]) for j in range(D)]
        if free:
            H = hamiltonian_on(model, K, Pn, sws, num(t2), [cls(x, zero) for x in X])
            miss.append(H.v if isinstance(H, fr.Dual) else H)
    return dict(xf=X, miss=miss, nupd=nupd, nskip=nskip, tf=t2, dxmax=dmax, xs=xs, samples=g)


NAMES = ("Xf", "miss", "nupd", "nskip", "tf", "dxmax", "Xs")


def pack(cases, B, Kc, M, D, cap, free, fill_bits, fill_int, tf=True, dxmax=True, xs=True):
    """What the call must leave in buffers filled with fill_bits / fill_int, in the order of NAMES: uint64 views of the doubles, int32
    counters; None for an output whose pointer is NULL.  cases[b][k] as guide_case returns them."""
    S, NM = 2 * D, D + 1 if free else D
    u = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)                        # noqa: E731
    full = lambda *shape: np.full(shape, np.uint64(fill_bits), dtype=np.uint64)                    # noqa: E731
    Xf, miss, T, dm, Xs = full(B, Kc, S), full(B, Kc, NM), full(B, Kc), full(B, Kc), full(B, Kc, M, cap, S)
    nupd, nskip = np.full((B, Kc), fill_int, dtype=np.int32), np.full((B, Kc), fill_int, dtype=np.int32)
    for b in range(B):
        for k in range(Kc):
            c = cases[b][k]
            Xf[b, k], miss[b, k] = u(c["xf"]), u(c["miss"])
            T[b, k], dm[b, k] = u([c["tf"]])[0], u([c["dxmax"]])[0]
            nupd[b, k], nskip[b, k] = c["nupd"], c["nskip"]
            for i in range(M):
                for q, x in enumerate(c["xs"][i][:cap]):
                    if x is not None:
                        Xs[b, k, i, q] = u(x)
    return Xf, miss, nupd, nskip, (T if tf else None), (dm if dxmax else None), (Xs if xs else None)
