"""socp_newton_batch restated in numpy (helper of test_newton_cpu.py / test_gpu_newton_batch.py, not a test).

The rounds of include/socp_hip.h ("Polishing a table of roots"), one operation per rounding: `polish` runs ONE row's state machine
on callables, with tangent_reference.eliminate for the solve; `newton_reference` builds the callables from restatements the tests
already have -- the CPU oracle's residual, its forward-difference Jacobian (the one branch_reference uses) and its variational
Jacobian, and exact_jacobian_reference for jac = 2.  A model without an oracle (the example plugins) takes its residual from the
value parts of exact_jacobian_reference and the forward differences of `fd_jacobian` (MINPACK's fdjac1, as the oracle writes it).
numpy multiplies and adds in separate roundings (no fused multiply-add), which is what the reference-order flavour of the device
kernels does.  A row's result depends on that row alone, so `newton_reference` computes equal rows once.

`mutate` names the WRONG restatements the CPU tests must catch: "no_ck" (the acceptance bar is rn, without c_k), "descending"
(the trials taken from the shortest step to the full one), "stale_f0" (F0 not refreshed after an accepted step)."""
import numpy as np

import tangent_reference as tr
from tangent_reference import F64

RUNNING, CONVERGED, SMALL_STEP, STALLED, SINGULAR, BAD_START = range(6)
STATUS_NAMES = ("RUNNING", "CONVERGED", "SMALL_STEP", "STALLED", "SINGULAR", "BAD_START")
DEFAULTS = dict(jac=2, epsfcn=1e-15, ftol=1e-12, xtol=0.0, trials=4, rounds=20)
MUTATIONS = ("no_ck", "descending", "stale_f0")


def options(**kw):
    """The options of a call as a dict; unknown names are refused."""
    assert set(kw) <= set(DEFAULTS), sorted(set(kw) - set(DEFAULTS))
    return dict(DEFAULTS, **kw)


def maxabs(x):
    """max_i |x_i|: a NaN when an entry is one, infinite when one is infinite and none is a NaN."""
    a = np.abs(np.asarray(x, dtype=F64))
    return F64(np.nan) if np.isnan(a).any() else (F64(a.max()) if a.size else F64(0.0))


def fd_jacobian(residual, z, F0, epsfcn):
    """MINPACK fdjac1 (dense): column j = (F(z + h e_j) - F0) / h with h = e |z_j|, or e when that is zero."""
    z = np.array(z, dtype=F64)
    e = tr.fd_step(epsfcn)
    J = np.zeros((len(z), len(z)))
    with np.errstate(all="ignore"):
        for j in range(len(z)):
            x = z.copy()
            h = e * abs(x[j])
            if h == 0:
                h = e
            x[j] = x[j] + h
            J[:, j] = (np.asarray(residual(x), dtype=F64) - F0) / h
    return J


def polish(residual, jacobian, z0, opts, mutate=()):
    """One row.  residual(z) -> F[n]; jacobian(z, F0) -> J[n][n] (J[i][j] = dF_i / dz_j).  Returns dict(z[n], f[n], rnorm, dnorm,
    iters, nhalf, status, rhist[rounds + 1]) and, beyond what the device reports, rounds_used."""
    assert set(mutate) <= set(MUTATIONS)
    o = options(**opts)
    trials, rounds, ftol, xtol = int(o["trials"]), int(o["rounds"]), F64(o["ftol"]), F64(o["xtol"])
    y = np.array(z0, dtype=F64)
    rhist = np.full(rounds + 1, np.nan)
    iters = nhalf = used = 0
    dnorm = F64(np.nan)
    with np.errstate(all="ignore"):
        F0 = np.asarray(residual(y), dtype=F64)
        rn = maxabs(F0)
        rhist[0] = rn
        Fj = F0                                                  # what the Jacobian and the right-hand side read
        status = BAD_START if not np.isfinite(rn) else (CONVERGED if rn <= ftol else RUNNING)
        for _ in range(rounds):
            if status != RUNNING:
                break
            used += 1
            J = np.asarray(jacobian(y, Fj), dtype=F64)
            delta, info, _ = tr.eliminate(J, (-Fj)[None, :])
            delta = delta[0]
            dn = maxabs(delta)
            if info != 0:
                status, dnorm = SINGULAR, F64(np.nan)
                break
            dnorm = dn
            order = range(trials - 1, -1, -1) if "descending" in mutate else range(trials)
            won = None
            for k in order:
                sk = F64(1.0) / F64(1 << k)
                t = y + sk * delta
                Fk = np.asarray(residual(t), dtype=F64)
                rk = maxabs(Fk)
                ck = F64(1.0) if "no_ck" in mutate else F64(1.0) - sk / F64(4.0)
                if rk < ck * rn:                                 # a NaN never passes
                    won = (k, sk, t, Fk, rk)
                    break
            if won is None:
                status = STALLED
                break
            k, sk, y, F0, rn = won
            if "stale_f0" not in mutate:
                Fj = F0
            iters += 1
            nhalf += k
            rhist[iters] = rn
            if rn <= ftol:
                status = CONVERGED
            elif xtol > 0 and sk * dn <= xtol * maxabs(y):
                status = SMALL_STEP
    return dict(z=y, f=F0, rnorm=float(rn), dnorm=float(dnorm), iters=iters, nhalf=nhalf, status=status, rhist=rhist, rounds_used=used)


def stack(rows):
    """The per-row dicts of `polish` as the arrays of the device call."""
    out = {}
    for key in ("z", "f", "rhist"):
        out[key] = np.array([r[key] for r in rows], dtype=F64)
    for key in ("rnorm", "dnorm"):
        out[key] = np.array([r[key] for r in rows], dtype=F64)
    for key in ("iters", "nhalf", "status", "rounds_used"):
        out[key] = np.array([r[key] for r in rows], dtype=np.int32)
    return out


_ROWS = {}


def row_callables(model, o, prob, nparams, N, block, pb, jac, epsfcn):
    """(residual, jacobian) of one row's setting: block[nparams + 2] and the Problem pb."""
    import exact_jacobian_reference as ej
    P, sw = [float(p) for p in block[:nparams]], (float(block[nparams]), float(block[nparams + 1]))

    def residual(z):
        z = np.ascontiguousarray(z, dtype=F64)
        if o is not None:
            return tr._residual(o, nparams, block, pb, z)
        return ej.exact_jacobian_row(model, P, sw, pb, z, N, derivs=False)[1]

    def jacobian(z, F0):
        z = np.ascontiguousarray(z, dtype=F64)
        if jac == 2:
            return ej.exact_jacobian_row(model, P, sw, pb, z, N)[0]
        if o is None:
            assert jac == 0
            return fd_jacobian(residual, z, F0, epsfcn)
        o.set_params(block[:nparams])
        o.m.sw[0], o.m.sw[1] = sw
        return o.fdjac(pb, z, np.ascontiguousarray(F0), epsfcn) if jac == 0 else o.jacobian(pb, z)

    return residual, jacobian


def newton_reference(model, o, prob, nparams, N, Z, opts, params=None, time=None, xnode=None, own=None, mutate=()):
    """The call for every row of Z.  model: the name exact_jacobian_reference knows ("goddard", "dint", "covid", "osc1d"); o: the CPU
    oracle set to the context's parameters, or None (then own = the context's packed block [nparams + 2]); N: the RK4 steps;
    params[B][nparams + 2] / time[B][M+1] / xnode[B][(M+1) 2d]: per-row blocks (None: the shared ones).  Returns the arrays of `stack`."""
    from oracle.oracle import Problem
    op = options(**opts)
    Z = np.asarray(Z, dtype=F64).reshape(-1, prob.n)
    s, M = 2 * prob.dim, prob.M
    if o is not None:
        keep, keep_sw = o.params().copy(), (o.m.sw[0], o.m.sw[1])
    rows = []
    try:
        for b, z in enumerate(Z):
            if o is not None:
                o.set_params(keep)
                o.m.sw[0], o.m.sw[1] = keep_sw
                block, pb = tr._row_setting(o, prob, nparams, b, params, time, xnode)
            else:
                block = np.array(params[b] if params is not None else own, dtype=F64)
                pb = Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time if time is None else time[b],
                             prob.xnode if xnode is None else np.asarray(xnode[b]).reshape(M + 1, s))
            key = (model, N, z.tobytes(), block.tobytes(), np.asarray(pb.time, dtype=F64).tobytes(), np.asarray(pb.xnode, dtype=F64).tobytes(),
                   np.asarray(prob.mode_t).tobytes(), np.asarray(prob.mode_x).tobytes(), tuple(sorted(op.items())), tuple(mutate))
            if key not in _ROWS:
                residual, jacobian = row_callables(model, o, prob, nparams, N, block, pb, int(op["jac"]), op["epsfcn"])
                _ROWS[key] = polish(residual, jacobian, z, op, mutate)
            rows.append(_ROWS[key])
    finally:
        if o is not None:
            o.set_params(keep)
            o.m.sw[0], o.m.sw[1] = keep_sw
    return stack(rows)
