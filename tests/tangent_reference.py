"""socp_tangent_batch restated in numpy on the CPU oracle (helper of test_tangent_cpu.py / test_gpu_tangent_batch.py, not a test).

Steps 1-6 of include/socp_hip.h, one operation per rounding: Oracle.residual with a moved parameter / Problem for the differences,
Oracle.fdjac (or Oracle.jacobian) for J, and the elimination loop as the header writes it.  numpy multiplies and subtracts in
separate roundings (no fused multiply-add), which is what the reference-order flavour of the device kernel does."""
import numpy as np

DIR_PARAM, DIR_TIME, DIR_XNODE = 0, 1, 2
F64 = np.float64
NAN_BITS = 0x7FF8000000000000


def fd_step(epsfcn):
    """e = sqrt(max(epsfcn, DBL_EPSILON)): MINPACK fdjac1's factor."""
    return float(np.sqrt(F64(max(float(epsfcn), float(np.finfo(F64).eps)))))


def moved(theta, e):
    """(theta + h, h) with h = e |theta|, or e when theta == 0.0."""
    theta = float(theta)
    h = e if theta == 0.0 else e * abs(theta)
    return theta + h, h


def eliminate(A, Y):
    """A[n][n] as a matrix A[i][j], Y[K][n] -> (X[K][n], info, swaps): Gaussian elimination with partial pivoting, the first
    maximum wins, a NaN below the diagonal is never chosen, a NaN on it stays; info = k + 1 and NaN rows when step k has no pivot
    (best not > 0, or infinite), n + 1 when a solution entry is not finite, else 0.  swaps: the number of steps with p != k."""
    A = np.array(A, dtype=F64)
    n = A.shape[0]
    W = np.array(Y, dtype=F64).reshape(-1, n).T.copy()          # right-hand sides as columns
    swaps = 0
    with np.errstate(all="ignore"):
        for k in range(n):
            col = np.abs(A[k:, k])
            if np.isnan(col[0]):
                best, p = col[0], k
            else:
                c = np.where(np.isnan(col), -1.0, col)
                p = k + int(np.argmax(c))                       # argmax: the first of equal maxima
                best = c[p - k]
            if not (best > 0.0) or np.isinf(best):
                return np.full((W.shape[1], n), np.nan), k + 1, swaps
            if p != k:
                A[[k, p]] = A[[p, k]]
                W[[k, p]] = W[[p, k]]
                swaps += 1
            l = A[k + 1:, k] / A[k, k]
            A[k + 1:, k] = l
            A[k + 1:, k + 1:] = A[k + 1:, k + 1:] - l[:, None] * A[k, k + 1:][None, :]
            W[k + 1:] = W[k + 1:] - l[:, None] * W[k][None, :]
        for k in range(n - 1, -1, -1):
            W[k] = W[k] / A[k, k]
            W[:k] = W[:k] - A[:k, k][:, None] * W[k][None, :]
    return W.T.copy(), (0 if np.all(np.isfinite(W)) else n + 1), swaps


def eliminate_batch(A, Y):
    """A[B][n][n] matrices, Y[B][K][n] -> (X[B][K][n], info[B])."""
    out = [eliminate(a, y) for a, y in zip(A, Y)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32)


def backward_error(J, dz, G):
    """max over the right-hand sides of ||J dz + G||inf / (||J||inf ||dz||inf + ||G||inf), evaluated in long double."""
    J, dz, G = (np.asarray(a, dtype=np.longdouble) for a in (J, dz, G))
    worst = 0.0
    for x, g in zip(dz.reshape(-1, J.shape[0]), G.reshape(-1, J.shape[0])):
        r = np.max(np.abs(J @ x + g))
        worst = max(worst, float(r / (np.max(np.sum(np.abs(J), axis=1)) * np.max(np.abs(x)) + np.max(np.abs(g)))))
    return worst


def _row_setting(o, prob, nparams, b, params, time, xnode):
    """(packed block [nparams + 2], Problem) of row b: its own blocks or the oracle's parameters / the shared problem."""
    from oracle.oracle import Problem
    block = np.array(params[b], dtype=F64) if params is not None else np.concatenate([o.params()[:nparams], [o.m.sw[0], o.m.sw[1]]])
    s, M = 2 * prob.dim, prob.M
    pb = Problem(prob.dim, prob.mode_t, prob.mode_x, prob.time if time is None else time[b],
                 prob.xnode if xnode is None else np.asarray(xnode[b]).reshape(M + 1, s))
    return block, pb


def _residual(o, nparams, block, pb, z):
    o.set_params(block[:nparams])
    o.m.sw[0], o.m.sw[1] = float(block[nparams]), float(block[nparams + 1])
    return o.residual(pb, z)


def tangent_reference(o, prob, nparams, Z, dirs, epsfcn=1e-15, jac=0, params=None, time=None, xnode=None, jacobians=None):
    """Steps 1-6 for every row of Z on the oracle `o` and the problem `prob`; params[B][nparams + 2] / time[B][M+1] /
    xnode[B][M+1][2d]: per-row blocks (None: the oracle's / the problem's own).  jacobians: None, or J[B][n][n] to use instead of
    the oracle's (the throughput-flavour checks feed the device's own).  Returns dict(dz[B][K][n], info[B], fp[B][K][n], J[B][n][n],
    swaps[B])."""
    from oracle.oracle import Problem
    Z = np.asarray(Z, dtype=F64).reshape(-1, prob.n)
    e = fd_step(epsfcn)
    own, own_sw = o.params().copy(), (o.m.sw[0], o.m.sw[1])
    s, M = 2 * prob.dim, prob.M
    out = dict(dz=[], info=[], fp=[], J=[], swaps=[])
    try:
        for b, z in enumerate(Z):
            block, pb = _row_setting(o, prob, nparams, b, params, time, xnode)
            F0 = _residual(o, nparams, block, pb, z)
            G = []
            for kind, index in dirs:
                blk, tt, xx = block.copy(), pb.time.copy(), pb.xnode.copy().ravel()
                target = {DIR_PARAM: blk, DIR_TIME: tt, DIR_XNODE: xx}[kind]
                target[index], h = moved(target[index], e)
                Fk = _residual(o, nparams, blk, Problem(prob.dim, prob.mode_t, prob.mode_x, tt, xx.reshape(M + 1, s)), z)
                G.append((Fk - F0) / h)
            G = np.array(G)
            o.set_params(block[:nparams])
            o.m.sw[0], o.m.sw[1] = float(block[nparams]), float(block[nparams + 1])
            if jacobians is not None:
                J = np.asarray(jacobians[b], dtype=F64)
            else:
                J = o.fdjac(pb, z, F0, epsfcn) if jac == 0 else o.jacobian(pb, z)
            dz, info, swaps = eliminate(J, -G)
            for key, val in (("dz", dz), ("info", info), ("fp", G), ("J", J), ("swaps", swaps)):
                out[key].append(val)
    finally:
        o.set_params(own)
        o.m.sw[0], o.m.sw[1] = own_sw
    return {k: np.array(v) for k, v in out.items()}


# ---- the second-order predictor check shared by the CPU and the GPU tests ----------------------------------------------------

def newton(residual, jacobian, z, iters=12, tol=1e-13):
    """Plain Newton polish: z <- z - J^-1 F until the step is below tol (1 + |z|); returns z."""
    z = np.array(z, dtype=F64)
    for _ in range(iters):
        dz = np.linalg.solve(jacobian(z), -residual(z))
        z = z + dz
        if np.max(np.abs(dz)) <= tol * (1.0 + np.max(np.abs(z))):
            break
    return z


def predictor_errors(solve_at, z0, dz, theta, fractions):
    """For theta' = theta (1 + f), f in fractions: (first-order errors ||z0 + (theta' - theta) dz - z*(theta')||2, zero-order errors
    ||z0 - z*(theta')||2); solve_at(theta', start) returns the re-solved z*(theta')."""
    first, zero = [], []
    for f in fractions:
        d = theta * f
        pred = z0 + d * dz
        zs = solve_at(theta + d, pred)
        first.append(float(np.linalg.norm(pred - zs)))
        zero.append(float(np.linalg.norm(z0 - zs)))
    return first, zero


def check_second_order(first, zero, what):
    """The predictor check both test files share: the first-order error falls by a factor inside [3.5, 4.5] per halving of the
    move and is at most 1/20 of the zero-order error; the figures are printed first."""
    ratios = [first[i] / first[i + 1] for i in range(len(first) - 1)]
    print("%s: first-order errors %s, zero-order %s, ratios %s" % (what, ["%.3e" % v for v in first], ["%.3e" % v for v in zero],
                                                                     ["%.3f" % r for r in ratios]))
    assert all(3.5 <= r <= 4.5 for r in ratios), (what, ratios)
    assert all(f <= z / 20.0 for f, z in zip(first, zero)), (what, first, zero)


# ---- the cases -----------------------------------------------------------------------------------------------------------------

_CACHE = {}


def cached(key, build):
    if key not in _CACHE:
        _CACHE[key] = build()
    return _CACHE[key]


def polished(o, prob, z):
    return newton(lambda x: o.residual(prob, x), lambda x: o.fdjac(prob, x, o.residual(prob, x)), z)


def dint_case():
    """events_cases.dint_basic with its golden row Newton-polished on the oracle; rows 1, 2 are the case's perturbed copies."""
    def build():
        import events_cases as ec
        c = dict(ec.case("dint_basic"))
        Z = np.array(c["Z"])
        Z[0] = polished(c["o"], c["prob"], Z[0])
        c["Z"], c["nparams"] = Z, 3
        return c
    return cached("dint", build)


def goddard_case():
    """goddard_c1_problem at N = 10 (KD = 310, mu2 = 0.2) with the golden stage-3 row Newton-polished on the oracle."""
    def build():
        import events_cases as ec
        from conftest import goddard_c1_problem
        o = ec.goddard_oracle(10)
        prob, _ = goddard_c1_problem(o)
        z = polished(o, prob, ec.goddard_stage3_row())
        return dict(model="goddard", o=o, prob=prob, N=10, Z=z[None, :], params=o.params()[:8], nparams=8)
    return cached("goddard", build)
