"""CPU: socp_branch_batch as tests/branch_reference.py restates it (include/socp_hip.h, "Past a fold") -- the instrument tested
without a GPU: a scalar model with a certain fold, the Goddard KD branch on the CPU oracle with every status required to OCCUR, and
the double integrator along a boundary value with both Jacobians.  test_gpu_branch_batch.py holds the device to this restatement
bit for bit."""
import numpy as np

import branch_reference as br
import tangent_reference as tr
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE

EPS = float(np.finfo(np.float64).eps)
FOLD = dict(dir=1, goal=-0.5, h0=0.1, hmax=0.2, ftol=1e-12)
# the Goddard KD branch: theta = 310 against costates of 1e-2, so lambda = KD / 310; ftol: the polished row has ||F||inf ~ 1e-13
GODDARD = dict(wtheta=310.0, dir=-1, goal=0.0, h0=0.1, hmax=0.4, max_corr=6, cap=40, rounds=200, ftol=1e-10)
KD = (DIR_PARAM, 2)


def fold_residual(z, a):
    return np.array([z[0] - 0.0, z[0] + z[1] * z[1] + a - 1.0])


def fold_jacobian(z, a, F0):
    return np.array([[1.0, 0.0], [1.0, 2.0 * z[1]]])


def check_fold(r, opts, what):
    """The analytic assertions on a followed fold1d row (shared with the GPU suite): r as branch_reference.follow returns it."""
    ftol, hmax, goal = opts["ftol"], opts["hmax"], opts["goal"]
    cnt = int(r["count"])
    pts = np.asarray(r["y"])[:cnt]
    print("%s: %d points, max theta %.6f, ifold %d, nreject %d" % (what, cnt, pts[:, 2].max(), int(r["ifold"]), int(r["nreject"])))
    assert int(r["status"]) == br.REACHED and int(r["nfold"]) == 1
    p0, a = pts[:, 1], pts[:, 2]
    assert int(r["ifold"]) == int(np.argmax(p0 < 0)) and p0[int(r["ifold"])] < 0 <= p0[int(r["ifold"]) - 1], "the first point with p0 < 0"
    assert np.all(np.abs(p0 * p0 + a - 1.0) <= ftol) and np.all(np.asarray(r["rnorm"])[:cnt] <= ftol)
    # two neighbours straddle p0 = 0, so one of them has |p0| <= hmax
    assert 1.0 - hmax * hmax - ftol <= a.max() <= 1.0 + ftol
    assert np.all(np.diff(p0) < 0), "p0 is strictly decreasing: the branch is followed through the fold, never back"
    assert a[-1] <= goal < a[-2]
    assert np.all(np.isnan(np.asarray(r["y"])[cnt:])) and np.all(np.isnan(np.asarray(r["ttheta"])[cnt:]))
    tth = np.asarray(r["ttheta"])[:cnt]
    assert np.all(tth[:int(r["ifold"])] > 0) and np.all(tth[int(r["ifold"]):] < 0), "dtheta/ds changes sign at the fold, once"
    zg = np.asarray(r["zgoal"])
    assert abs(zg[0]) <= ftol and abs(zg[1] + np.sqrt(1.0 - goal)) <= hmax * hmax, "linear interpolation between the last two points"


def test_scalar_fold_is_passed():
    for dtheta in (None, lambda z, a, F0: np.array([0.0, 1.0])):
        r = br.follow(fold_residual, fold_jacobian, dtheta, [0.0, 1.0], 0.0, FOLD)
        check_fold(r, br.options(**FOLD), "scalar fold (%s dF/dtheta)" % ("differenced" if dtheta is None else "analytic"))


def goddard_run(**kw):
    g = tr.goddard_case()
    key = ("branch", tuple(sorted(kw.items())))
    return tr.cached(key, lambda: br.branch_reference(g["o"], g["prob"], 8, g["Z"], KD, dict(GODDARD, **kw)))


def test_goddard_kd_branch_to_zero_has_no_fold():
    g = tr.goddard_case()
    o, prob, n = g["o"], g["prob"], g["prob"].n
    r = goddard_run()
    cnt = int(r["count"][0])
    pts = r["y"][0, :cnt]
    print("goddard KD 310 -> 0: %d points, %d rounds, thetas %s" % (cnt, r["rounds_used"][0], np.round(pts[:, n], 2).tolist()))
    assert r["status"][0] == br.REACHED and r["nfold"][0] == 0 and r["ifold"][0] == -1 and r["nreject"][0] == 0
    assert np.all(np.diff(pts[:, n]) < 0) and pts[0, n] == 310.0 and pts[-1, n] <= 0.0 < pts[-2, n]
    own = o.params().copy()
    try:
        for i, p in enumerate(pts):
            q = own.copy()
            q[2] = p[n]
            o.set_params(q)
            F = o.residual(prob, np.ascontiguousarray(p[:n]))
            assert np.max(np.abs(F)) == r["rnorm"][0, i] <= GODDARD["ftol"], i
    finally:
        o.set_params(own)
    assert np.all(np.isfinite(r["zgoal"][0]))
    # point 0's tangent is parallel to the tangent call's: dz/dlambda = wtheta dz/dtheta
    t = tr.tangent_reference(o, prob, 8, g["Z"], [KD])
    first = br.branch_reference(o, prob, 8, g["Z"], KD, dict(GODDARD, rounds=1))
    assert first["status"][0] == br.RUNNING and first["count"][0] == 1
    t0 = first["t"][0]
    assert t0[n] == first["ttheta"][0, 0] < 0, "dir = -1: towards smaller KD"
    assert abs(np.linalg.norm(t0) - 1.0) <= 4 * (n + 1) * EPS
    want = GODDARD["wtheta"] * t["dz"][0, 0]
    cond = np.linalg.cond(t["J"][0])
    dev = np.max(np.abs(t0[:n] / t0[n] - want)) / np.max(np.abs(want))
    print("goddard: point 0 tangent against tangent_batch: %.3e (bar 1e3 eps cond2(J) = %.3e, cond %.3e)" % (dev, 1e3 * EPS * cond, cond))
    assert dev <= 1e3 * EPS * cond


def test_goddard_every_other_status_occurs():
    n = 85
    r = goddard_run(h0=6.4, hmax=6.4, max_corr=3)
    assert r["status"][0] == br.REACHED and r["nreject"][0] >= 1 and r["nfold"][0] == 0
    r = goddard_run(h0=0.4, hmax=0.4, max_corr=1, cap=40)
    assert r["status"][0] == br.FULL and r["nreject"][0] >= 1 and r["count"][0] == 40 and np.all(np.isfinite(r["y"][0]))
    assert np.all(np.isnan(r["zgoal"][0]))
    r = goddard_run(h0=8.0, hmax=8.0, hmin=3.0, max_corr=2)
    assert r["status"][0] == br.STEP_TOO_SMALL and r["count"][0] == 1 and r["hlast"][0] < 3.0 and np.all(np.isnan(r["y"][0, 1:]))
    r = goddard_run(rounds=5)
    assert r["status"][0] == br.RUNNING and 1 <= r["count"][0] < 5 and r["rounds_used"][0] == 5
    full = goddard_run()
    k = int(r["count"][0])
    assert np.array_equal(r["y"][0, :k], full["y"][0, :k]), "a RUNNING row's accepted points are the full run's"
    g = tr.goddard_case()
    Z = np.array(g["Z"])
    Z[0, 17] = np.nan
    r = br.branch_reference(g["o"], g["prob"], 8, Z, KD, GODDARD)
    assert r["status"][0] == br.BAD_START and r["count"][0] == 0 and np.all(np.isnan(r["y"][0])) and r["hlast"][0] == GODDARD["h0"]
    # a direction the model ignores -- the time entry of the FREE end node: g = 0 and the last row is e_{n+1}^T, so the tangent is
    # (0, .., 0, -1) exactly: z never moves, every predictor is accepted as it stands, theta walks down by h wtheta with h doubling
    opts = dict(GODDARD, goal=None, cap=6, wtheta=1.0)
    r = br.branch_reference(g["o"], g["prob"], 8, g["Z"], (DIR_TIME, g["prob"].M), opts)
    assert r["status"][0] == br.FULL and r["count"][0] == 6 and r["nreject"][0] == 0 and r["nfold"][0] == 0
    assert np.all(r["y"][0, :, :n] == g["Z"][0]) and np.all(r["ttheta"][0] == -1.0) and np.all(r["rnorm"][0] == r["rnorm"][0, 0])
    theta0 = g["prob"].time[g["prob"].M]
    want = theta0 - np.concatenate([[0.0], np.cumsum([0.1, 0.2, 0.4, 0.4, 0.4])])
    assert np.max(np.abs(r["y"][0, :, n] - want)) <= 8 * EPS * abs(theta0) and r["hlast"][0] == 0.4


def test_double_integrator_boundary_value_with_both_jacobians():
    c = tr.dint_case()
    o, prob, n = c["o"], c["prob"], c["prob"].n
    d = (DIR_XNODE, 12)                                          # the final position: xnode[1][0] = 10
    assert prob.xnode[1, 0] == 10.0
    z0 = c["Z"][:1]
    # what the difference of the two Jacobians does to the tangent of point 0, by numpy alone (wtheta = 1).  The norm of the
    # difference itself says nothing here: the columns of the fixed initial states differ by O(1) between the two, and no tangent
    # has a component along them
    tan = tr.tangent_reference(o, prob, 3, z0, [d], jac=1)
    J_fd = o.fdjac(prob, z0[0], o.residual(prob, z0[0]), 1e-15)
    unit = np.zeros(n + 1)
    unit[n] = 1.0
    tangents = []
    for J in (J_fd, tan["J"][0]):
        M0 = np.vstack([np.hstack([J, tan["fp"][0, 0][:, None]]), unit[None, :]])
        tau = np.linalg.solve(M0, unit)
        tangents.append(tau / np.linalg.norm(tau))
    rel = float(np.linalg.norm(tangents[0] - tangents[1]))
    inv_norm = np.linalg.norm(np.linalg.inv(M0), 2)
    for goal, direction in ((14.0, 1), (-4.0, -1)):
        opts = dict(dir=direction, goal=goal, h0=1.0, hmax=4.0, ftol=1e-9, cap=32, rounds=200)
        runs = [br.branch_reference(o, prob, 3, z0, d, dict(opts, jac=jac)) for jac in (0, 1)]
        for r in runs:
            cnt = int(r["count"][0])
            th = r["y"][0, :cnt, n]
            assert r["status"][0] == br.REACHED and r["nfold"][0] == 0 and np.all(np.diff(th) * direction > 0)
            assert (th[-1] - goal) * direction >= 0 > (th[-2] - goal) * direction and np.all(np.isfinite(r["zgoal"][0]))
        assert runs[0]["count"][0] == runs[1]["count"][0]
        cnt = int(runs[0]["count"][0])
        a, b = runs[0]["y"][0, :cnt], runs[1]["y"][0, :cnt]
        length = float(np.sum(np.linalg.norm(np.diff(b, axis=0), axis=1)))
        dev = float(np.max(np.abs(a - b)))
        # each tangent differs by ~rel, each step is at most hmax long: the paths part by at most rel x the length walked (x 10)
        bar = 10.0 * (rel * length + opts["ftol"] * inv_norm)
        print("dint xnode 10 -> %g: %d points, paths differ by %.3e (bar %.3e; tangents of point 0 differ by %.3e, length %.2f)" % (goal, cnt, dev, bar, rel, length))
        assert dev <= bar
        if goal < 0:
            assert np.any(th[:-1] > 0) and th[-1] < 0, "theta passes 0, where the step rule of the differences changes"
