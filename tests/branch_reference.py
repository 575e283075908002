"""socp_branch_batch restated in numpy (helper of test_branch_cpu.py / test_gpu_branch_batch.py, not a test).

The rounds of include/socp_hip.h ("Past a fold"), one operation per rounding: `follow` runs ONE row's state machine on callables,
with tangent_reference.eliminate for every solve and tangent_reference.fd_step / moved for the parameter step; `branch_reference`
builds the callables on the CPU oracle the way tangent_reference.tangent_reference does.  numpy multiplies and adds in separate
roundings (no fused multiply-add), which is what the reference-order flavour of the device kernels does."""
import numpy as np

import tangent_reference as tr
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE, F64

RUNNING, REACHED, FULL, STEP_TOO_SMALL, SINGULAR, BAD_START = range(6)
DEFAULTS = dict(epsfcn=1e-15, jac=0, wtheta=1.0, dir=1, h0=0.1, hmin=1e-8, hmax=1.0, grow=2.0, kfast=2, max_corr=6, ftol=1e-10,
                goal=None, cap=64, rounds=200)


def options(**kw):
    """The options of a call as a dict (goal=None: no goal); unknown names are refused."""
    assert set(kw) <= set(DEFAULTS), sorted(set(kw) - set(DEFAULTS))
    return dict(DEFAULTS, **kw)


def seqnorm2(x):
    """sum x_i^2, one rounded product added at a time from +0.0."""
    s = F64(0.0)
    for xi in x:
        s = s + F64(xi) * F64(xi)
    return s


def follow(residual, jacobian, dtheta, z0, theta0, opts):
    """One row.  residual(z, theta) -> F[n]; jacobian(z, theta, F0) -> J[n][n]; dtheta: None (g is differenced from `residual` with
    the step of tangent_reference.moved, as the device does), or dtheta(z, theta, F0) -> dF/dtheta[n] before the scale.  Returns
    dict(y[cap][n+1], ttheta[cap], rnorm[cap], count, nfold, ifold, status, nreject, hlast, zgoal[n]) and, beyond what the device
    reports, rounds_used and t[n+1]: the unit tangent the row holds at the end."""
    o = options(**opts)
    n, cap, w = len(z0), int(o["cap"]), F64(o["wtheta"])
    n1 = n + 1
    e = tr.fd_step(o["epsfcn"])
    have_goal, goal = o["goal"] is not None, F64(0.0 if o["goal"] is None else o["goal"])
    hmin, hmax, grow, ftol = F64(o["hmin"]), F64(o["hmax"]), F64(o["grow"]), F64(o["ftol"])
    Y = np.full((cap, n1), np.nan)
    ttheta, rnorm, zgoal = np.full(cap, np.nan), np.full(cap, np.nan), np.full(n, np.nan)
    count = nfold = nreject = 0
    ifold, status = -1, RUNNING
    v = np.concatenate([np.asarray(z0, dtype=F64), [F64(theta0) / w]])
    y, t = v.copy(), np.zeros(n1)
    h, k, used = F64(o["h0"]), 0, 0
    unit = np.zeros(n1)
    unit[n] = 1.0
    with np.errstate(all="ignore"):
        for rnd in range(int(o["rounds"])):
            if status != RUNNING:
                break
            used += 1
            first = rnd == 0
            theta = float(v[n] * w)
            F0 = np.asarray(residual(v[:n], theta), dtype=F64)
            if dtheta is None:
                thm, hth = tr.moved(theta, e)
                g = ((np.asarray(residual(v[:n], thm), dtype=F64) - F0) / F64(hth)) * w
            else:
                g = np.asarray(dtheta(v[:n], theta, F0), dtype=F64) * w
            J = np.asarray(jacobian(v[:n], theta, F0), dtype=F64)
            rn = np.max(np.abs(F0))                              # a NaN when an entry is one
            M = np.zeros((n1, n1))
            M[:n, :n], M[:n, n] = J, g
            if first:
                M[n, n] = F64(o["dir"])                          # the other entries of the row are +0.0
            else:
                M[n] = t
            predict = reject = False
            if first or rn <= ftol:                              # start / accept
                if first and not np.isfinite(rn):
                    status = BAD_START
                    break
                y = v.copy()
                tau, info, _ = tr.eliminate(M, unit[None, :])
                s = seqnorm2(tau[0])
                singular = info != 0 or s == 0.0 or not np.isfinite(s)
                idx = count
                Y[idx, :n], Y[idx, n], rnorm[idx] = v[:n], theta, rn
                count += 1
                if singular:
                    status = SINGULAR
                    break
                tnew = tau[0] / np.sqrt(s)
                ttheta[idx] = tnew[n]
                if first:
                    t, h, predict = tnew, F64(o["h0"]), True
                else:
                    if np.signbit(tnew[n]) != np.signbit(t[n]):
                        nfold += 1
                        if ifold < 0:
                            ifold = idx
                    if k <= int(o["kfast"]):
                        h = min(h * grow, hmax)
                    t = tnew
                    reached = False
                    if have_goal:
                        tp = Y[idx - 1, n]
                        a, b = tp - goal, F64(theta) - goal
                        reached = bool(b == 0.0 or (a != 0.0 and (a < 0.0) != (b < 0.0)))
                        if reached:
                            sc = (goal - tp) / (F64(theta) - tp)
                            zgoal = Y[idx - 1, :n] + sc * (v[:n] - Y[idx - 1, :n])
                    if reached:
                        status = REACHED
                    elif count == cap:
                        status = FULL
                    else:
                        predict = True
            elif not np.isfinite(rn) or k == int(o["max_corr"]):
                reject = True
            else:                                                # correct
                delta, info, _ = tr.eliminate(M, np.concatenate([-F0, [0.0]])[None, :])
                dn = np.sqrt(seqnorm2(delta[0]))
                if info != 0 or not (dn <= h):
                    reject = True
                else:
                    v = v + delta[0]
                    k += 1
            if reject:
                nreject += 1
                h = h / F64(2.0)
                if h < hmin:
                    status = STEP_TOO_SMALL
                else:
                    predict = True
            if predict:
                v = y + h * t
                k = 0
    return dict(y=Y, ttheta=ttheta, rnorm=rnorm, count=count, nfold=nfold, ifold=ifold, status=status, nreject=nreject, hlast=float(h),
                zgoal=zgoal, rounds_used=used, t=np.array(t))


def stack(rows):
    """The per-row dicts of `follow` as the arrays of the device call."""
    out = {}
    for key in ("y", "ttheta", "rnorm", "zgoal", "t"):
        out[key] = np.array([r[key] for r in rows], dtype=F64)
    out["hlast"] = np.array([r["hlast"] for r in rows], dtype=F64)
    for key in ("count", "nfold", "ifold", "status", "nreject", "rounds_used"):
        out[key] = np.array([r[key] for r in rows], dtype=np.int32)
    return out


def branch_reference(o, prob, nparams, Z, dir, opts, params=None, time=None, xnode=None):
    """The rounds for every row of Z on the oracle `o` and the problem `prob`, along dir = (kind, index); params[B][nparams + 2] /
    time[B][M+1] / xnode[B][M+1][2d]: per-row blocks (None: the oracle's / the problem's own).  Returns the arrays of `stack`."""
    from oracle.oracle import Problem
    kind, index = dir
    op = options(**opts)
    Z = np.asarray(Z, dtype=F64).reshape(-1, prob.n)
    own, own_sw = o.params().copy(), (o.m.sw[0], o.m.sw[1])
    s, M = 2 * prob.dim, prob.M
    rows = []
    try:
        for b, z in enumerate(Z):
            o.set_params(own)                                    # the callables below leave the last point's block in the oracle
            o.m.sw[0], o.m.sw[1] = own_sw
            block, pb = tr._row_setting(o, prob, nparams, b, params, time, xnode)

            def setting(theta):
                blk, tt, xx = block.copy(), pb.time.copy(), pb.xnode.copy().ravel()
                {DIR_PARAM: blk, DIR_TIME: tt, DIR_XNODE: xx}[kind][index] = theta
                return blk, Problem(prob.dim, prob.mode_t, prob.mode_x, tt, xx.reshape(M + 1, s))

            def residual(zz, theta):
                blk, p = setting(theta)
                return tr._residual(o, nparams, blk, p, np.ascontiguousarray(zz))

            def jacobian(zz, theta, F0):
                blk, p = setting(theta)
                o.set_params(blk[:nparams])
                o.m.sw[0], o.m.sw[1] = float(blk[nparams]), float(blk[nparams + 1])
                zz = np.ascontiguousarray(zz)
                return o.fdjac(p, zz, F0, op["epsfcn"]) if op["jac"] == 0 else o.jacobian(p, zz)

            theta0 = {DIR_PARAM: block, DIR_TIME: pb.time, DIR_XNODE: pb.xnode.ravel()}[kind][index]
            rows.append(follow(residual, jacobian, None, z, theta0, op))
    finally:
        o.set_params(own)
        o.m.sw[0], o.m.sw[1] = own_sw
    return stack(rows)
