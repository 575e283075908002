"""GPU: the Hamiltonian gradient (socp_hamiltonian_gradient_batch[_dev], capi.Context.hamiltonian_gradient_batch) and the models
written from their Hamiltonian alone (tests/plugin/osc1d_h_plugin.hip, dint_h_plugin.hip) against tests/hamiltonian_model_reference.py
-- the definition restated in Python on dual numbers.  Outputs live in sentinel-filled buffers followed by 64 guard words and are
compared WHOLE on integer views (the conventions of test_gpu_exact_jacobian.py), so a store past the last row shows, and so does the
sign of a zero.  Every output is bit-equal to the restatement, in both flavours (the kernels are one object without contraction).
A reference is computed once, for 130 points, and its leading rows serve the smaller batches.  The figures the tests print are kept
in profiles/hamiltonian_model_gpu_tests.txt.  Without the feature every test fails: the symbol, the table entry and the plugins do
not exist."""
import ctypes as C

import numpy as np
import pytest

import hamiltonian_model_reference as hm
import jacobi_cases as jc
import test_hamiltonian_model_cpu as cpu
from test_gpu_jacobi_batch import SENT, GUARD, DP, sentinel, canon, plugin_path   # noqa: F401

pytestmark = pytest.mark.gpu
B_ALL = 130
SIZES = (1, 63, 64, 65, 130)
PLUGIN_IDS = {"lqr1d": 1001, "osc1d_exact_jacobian": 1005, "osc1d_h": 1008, "dint_h": 1009}
SW_CTX = (0.04, 0.12)                       # the context's own switching times: read where sw is NULL


def context(model, params, variant="exact", N=20):
    from socp_amd import capi
    if model in PLUGIN_IDS:
        capi.plugin_load(plugin_path(model))
        ctx = capi.Context(PLUGIN_IDS[model], nparams=len(params))
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[model])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(np.asarray(params, dtype=np.float64))
    ctx.set_step_number(N)
    ctx.set_switching_times(SW_CTX)
    return ctx


# ---- the points: name -> (device model, restated model, P, t[B], sw[B][2] or None, X[B][S]) ---------------------------------------

def goddard_points(mu2, own_sw):
    rng = np.random.default_rng(41)
    _, P, _, _, _ = cpu.points("goddard mu2=1")
    P = list(P)
    P[6] = mu2
    X, t = cpu.goddard_rows(rng, B_ALL, cpu.SW)
    X[:, 13] *= rng.choice([-10.0, 0.5, 1.0, 4.0], size=B_ALL)
    sw = np.array(cpu.SW) + rng.uniform(-0.02, 0.02, size=(B_ALL, 2)) if own_sw else None
    return "goddard", "goddard", P, t, sw, X


def covid_points():
    rng = np.random.default_rng(42)
    X = np.array([cpu.covid_state(c, a) for c in ("min", None, "max", None) for a in (False, True)] * 17)[:B_ALL]
    X = X * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=X.shape))
    return "covid", "covid", cpu.COVID_P, np.zeros(B_ALL), None, X


def dint_points(device="dint"):
    rng = np.random.default_rng(43)
    X = rng.uniform(-1.0, 1.0, size=(B_ALL, 12)) * rng.choice([0.3, 3.0], size=(B_ALL, 1))
    return device, "dint", cpu.DINT_P, rng.uniform(0.0, 1.0, size=B_ALL), None, X


def osc1d_points(device="osc1d_exact_jacobian"):
    rng = np.random.default_rng(44)
    X = rng.uniform(0.2, 1.0, size=(B_ALL, 2)) * rng.choice([-1.0, 1.0], size=(B_ALL, 2))
    return device, "osc1d", [4.0], np.zeros(B_ALL), None, X


POINTS = {"goddard smooth": lambda: goddard_points(1.0, False), "goddard general": lambda: goddard_points(0.0, True),
          "goddard general, context sw": lambda: goddard_points(0.0, False), "dint": dint_points, "covid": covid_points,
          "osc1d plugin": osc1d_points}
_POINTS, _REF = {}, {}


def points(name):
    if name not in _POINTS:
        _POINTS[name] = POINTS[name]()
        _REF[name] = None
    return _POINTS[name]


def reference(name):
    """G[130][S] of the restatement, computed once."""
    device, model, P, t, sw, X = points(name)
    if _REF.get(name) is None:
        _REF[name] = hm.gradient_batch(model, P, t, X, sw=sw, sw_default=SW_CTX)
        _REF[name].setflags(write=False)
        assert np.all(np.isfinite(_REF[name]))
    return _REF[name]


# ---- the two forms on guarded buffers: each returns the WHOLE buffer as an integer view ----------------------------------------

def run_host(ctx, t, sw, X):
    t, X = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64)
    sw = np.ascontiguousarray(sw, dtype=np.float64) if sw is not None else None
    out = sentinel(X.size)
    ctx._chk(ctx.L.socp_hamiltonian_gradient_batch(ctx.h, len(X), t.ctypes.data_as(DP), sw.ctypes.data_as(DP) if sw is not None else None,
                                                   X.ctypes.data_as(DP), out.ctypes.data_as(DP)))
    return out.view(np.uint64)


def run_dev(ctx, t, sw, X):
    import torch
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()                 # noqa: E731
    dt, dX, dsw = up(t), up(X), (up(sw) if sw is not None else None)
    dG = torch.from_numpy(sentinel(np.asarray(X).size)).cuda()
    torch.cuda.synchronize()
    ctx.hamiltonian_gradient_batch_dev(len(X), dt.data_ptr(), dsw.data_ptr() if dsw is not None else None, dX.data_ptr(), dG.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    return dG.cpu().numpy().view(np.uint64)


def check_whole(got, want, what):
    w = np.ascontiguousarray(want, dtype=np.float64).ravel().view(np.uint64)
    assert got.size == w.size + GUARD
    assert np.all(got[w.size:] == np.uint64(SENT)), "%s: guard words behind G were written" % what
    gg, ww = canon(got[:w.size]), canon(w)
    bad = np.argwhere(gg != ww).ravel()
    assert len(bad) == 0, (what, "%d differ; first flat indices:" % len(bad), bad[:5].tolist(), gg[bad[:5]].view(np.float64), ww[bad[:5]].view(np.float64))


# ---- 1. the gradient call, every model, sizes, forms --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(POINTS))
def test_gradient_equals_the_restatement(name):
    device, model, P, t, sw, X = points(name)
    want = reference(name)
    ctx = context(device, P)
    assert ctx.has_hamiltonian_gradient() and ctx.L.socp_ctx_has_hamiltonian_gradient(ctx.h) == 1
    t0, l0 = ctx.counters()
    for B in SIZES:
        cut = (t[:B], sw[:B] if sw is not None else None, X[:B])
        check_whole(run_host(ctx, *cut), want[:B], "%s, B = %d, host form" % (name, B))
        check_whole(run_dev(ctx, *cut), want[:B], "%s, B = %d, _dev form" % (name, B))
    t1, l1 = ctx.counters()
    assert (t1 - t0, l1 - l0) == (0, 2 * len(SIZES)), "one launch per call, no trajectory"
    G = ctx.hamiltonian_gradient_batch(t, X, sw=sw)
    assert np.array_equal(G.view(np.uint64), want.view(np.uint64)), "the Python binding"
    rhs = ctx.eval_batch(0, t, X, sw=sw)
    miss = np.max(np.abs(G - rhs), axis=0) / max(1.0, np.max(np.abs(rhs)))
    print("%-28s max |G - SOCP_EVAL_RHS| / max(1, |rhs|) by row: %s" % (name, " ".join("%.1e" % m for m in miss)))
    if model == "covid":
        assert np.all(miss[[4, 6]] > 1e-3) and np.all(miss[[0, 1, 2, 3, 5, 7]] < 1e-13), "covid19: rows 4 and 6, and only they"
    elif name.startswith("goddard general"):
        s0, s1 = (sw[:, 0], sw[:, 1]) if sw is not None else SW_CTX
        arc = np.where(t <= s0, 0, np.where(t <= s1, 1, 2))
        assert {0, 1, 2} == set(arc.tolist()), "all three arcs of the general law"
        off = np.max(np.abs(G - rhs), axis=1) / np.maximum(1.0, np.max(np.abs(rhs), axis=1))
        assert np.all(off[arc != 1] < 1e-12), "full thrust and thrust off: a minimising law"
        assert np.any(off[arc == 1] > 1e-3), "the closed-form singular control off the singular surface is no minimiser (the CPU finding)"
    else:
        assert np.all(miss < 1e-12)
    ctx.close()


def test_goddard_takes_the_law_from_the_contexts_mu2():
    """The general-law kernel with mu2 = 0 and the smooth-law kernel with mu2 = 1 give different numbers at the same points."""
    a, b = reference("goddard smooth"), reference("goddard general, context sw")
    assert not np.array_equal(a, b)


@pytest.mark.parametrize("name", ["goddard smooth", "goddard general", "dint", "covid"])
def test_throughput_flavour_returns_the_same_bits(name):
    device, model, P, t, sw, X = points(name)
    ctx = context(device, P, "fast")
    assert ctx.has_hamiltonian_gradient()
    for B in (65, 130):
        check_whole(run_dev(ctx, t[:B], sw[:B] if sw is not None else None, X[:B]), reference(name)[:B], "%s, throughput flavour, B = %d" % (name, B))
    check_whole(run_host(ctx, t[:63], sw[:63] if sw is not None else None, X[:63]), reference(name)[:63], name + ", throughput flavour, host form")
    ctx.close()


# ---- 2. refusals and conventions ---------------------------------------------------------------------------------------------------

def test_refusals_and_conventions():
    import torch
    from socp_amd import capi
    device, model, P, t, sw, X = points("dint")
    B = 5
    t, X = np.ascontiguousarray(t[:B]), np.ascontiguousarray(X[:B])
    ctx = context(device, P)
    L, h = ctx.L, ctx.h
    out = sentinel(X.size)
    fresh = lambda a: bool(np.all(a.view(np.uint64) == np.uint64(SENT)))                   # noqa: E731
    dt, dX, dG = torch.from_numpy(t).cuda(), torch.from_numpy(X).cuda(), torch.from_numpy(sentinel(X.size)).cuda()
    torch.cuda.synchronize()
    c0 = ctx.counters()
    tp, Xp, Gp = t.ctypes.data_as(DP), X.ctypes.data_as(DP), out.ctypes.data_as(DP)
    assert L.socp_hamiltonian_gradient_batch(h, -1, tp, None, Xp, Gp) == capi.ERR_ARG and "B >= 0" in L.socp_last_error(h).decode()
    assert L.socp_hamiltonian_gradient_batch_dev(h, -1, dt.data_ptr(), None, dX.data_ptr(), dG.data_ptr()) == capi.ERR_ARG
    for args in ((None, None, Xp, Gp), (tp, None, None, Gp), (tp, None, Xp, None)):
        assert L.socp_hamiltonian_gradient_batch(h, B, *args) == capi.ERR_ARG
    for args in ((None, None, dX.data_ptr(), dG.data_ptr()), (dt.data_ptr(), None, None, dG.data_ptr()), (dt.data_ptr(), None, dX.data_ptr(), None)):
        assert L.socp_hamiltonian_gradient_batch_dev(h, B, *args) == capi.ERR_ARG
    assert L.socp_hamiltonian_gradient_batch(h, 0, None, None, None, None) == capi.OK, "B = 0"
    assert L.socp_hamiltonian_gradient_batch_dev(h, 0, None, None, None, None) == capi.OK
    assert L.socp_hamiltonian_gradient_batch(None, B, tp, None, Xp, Gp) == capi.ERR_ARG and L.socp_ctx_has_hamiltonian_gradient(None) == capi.ERR_ARG
    torch.cuda.synchronize()
    assert ctx.counters() == c0 and fresh(out) and fresh(dG.cpu().numpy()), "nothing was launched, counted or written"
    ctx.close()

    # models without the entry: the interceptor, vtolUAV and a plugin without hamiltonian_t
    gold = np.load(jc.os.path.join(jc.ROOT, "tests", "golden", "vtol_vectors.npz"))
    others = []
    ci = capi.Context(capi.MODEL_INTERCEPTOR)
    others.append(("interceptor", ci))
    cv = capi.Context(capi.MODEL_VTOLUAV)
    cv.set_map(gold["table_shipped"])
    others.append(("vtolUAV", cv))
    capi.plugin_load(plugin_path("lqr1d"))
    others.append(("lqr1d plugin", capi.Context(PLUGIN_IDS["lqr1d"], nparams=1)))
    for label, cx in others:
        S = cx.s
        assert not cx.has_hamiltonian_gradient() and cx.L.socp_ctx_has_hamiltonian_gradient(cx.h) == 0, label
        Xo, to, oo = np.full((3, S), 0.5), np.zeros(3), sentinel(3 * S)
        dXo, dto, doo = torch.from_numpy(Xo).cuda(), torch.from_numpy(to).cuda(), torch.from_numpy(sentinel(3 * S)).cuda()
        torch.cuda.synchronize()
        c0 = cx.counters()
        assert cx.L.socp_hamiltonian_gradient_batch(cx.h, 3, to.ctypes.data_as(DP), None, Xo.ctypes.data_as(DP), oo.ctypes.data_as(DP)) == capi.ERR_UNSUPPORTED
        assert "no hamiltonian_gradient entry" in cx.L.socp_last_error(cx.h).decode(), label
        assert cx.L.socp_hamiltonian_gradient_batch_dev(cx.h, 3, dto.data_ptr(), None, dXo.data_ptr(), doo.data_ptr()) == capi.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert cx.counters() == c0 and fresh(oo) and fresh(doo.cpu().numpy()), label
        with pytest.raises(capi.SocpError) as e:
            cx.hamiltonian_gradient_batch(to, Xo)
        assert e.value.code == capi.ERR_UNSUPPORTED
        cx.close()


# ---- 3. the models written from their Hamiltonian alone ----------------------------------------------------------------------------

H_MODELS = {"osc1d_h": lambda: osc1d_points("osc1d_h"), "dint_h": lambda: dint_points("dint_h")}


@pytest.mark.parametrize("name", list(H_MODELS))
def test_h_only_evaluations_equal_the_restatement(name):
    from socp_amd import capi
    device, base, P, t, sw, X = H_MODELS[name]()
    B = 65
    t, X = t[:B], X[:B]
    ctx = context(device, P)
    want = hm.gradient_batch(base, P, t, X, sw_default=SW_CTX)
    rhs = ctx.eval_batch(capi.EVAL_RHS, t, X)
    assert np.array_equal(rhs.view(np.uint64), want.view(np.uint64)), "SOCP_EVAL_RHS is the restated gradient"
    assert np.array_equal(want.view(np.uint64), np.array([hm.plain_rhs(name, P, SW_CTX, t[b], X[b]) for b in range(B)]).view(np.uint64))
    H = ctx.eval_batch(capi.EVAL_HAMILTONIAN, t, X)[:, 0]
    assert np.array_equal(H.view(np.uint64), np.array([hm.plain_hamiltonian(name, P, SW_CTX, t[b], X[b]) for b in range(B)]).view(np.uint64)), "plain H"
    check_whole(run_host(ctx, t, None, X), want, name + ": the gradient call on an H-only model")
    assert ctx.has_hamiltonian_gradient()
    assert not ctx.has_fields() and not ctx.has_exact_jacobian() and not ctx.has_sensitivity() and not ctx.has_variational(), "no rhs_t"
    assert [ctx.L.socp_ctx_has_fields(ctx.h), ctx.L.socp_ctx_has_exact_jacobian(ctx.h), ctx.L.socp_ctx_has_sensitivity(ctx.h),
            ctx.L.socp_ctx_has_variational(ctx.h)] == [0, 0, 0, 0]
    ctx.close()


@pytest.mark.parametrize("name", list(H_MODELS))
def test_h_only_trajectories_equal_numpy_rk4_on_the_restatement(name):
    device, base, P, t, sw, X = H_MODELS[name]()
    B, N, T = 65, 20, 1.5
    X = X[:B]
    ctx = context(device, P, N=N)
    Xf = ctx.integrate_batch(0.0, T, X)
    want = np.array([hm.integrate(name, P, SW_CTX, 0.0, T, X[b], N)[-1] for b in range(B)])
    assert np.isfinite(want).all()
    assert np.array_equal(Xf.view(np.uint64), want.view(np.uint64)), "integrate_batch, 20 steps, B = 65"
    if name == "dint_h":
        u = -X[:, 9:12] / P[1]
        sat = np.sqrt(np.sum(u * u, axis=1)) > P[0]
        assert sat.any() and not sat.all(), "both sides of the saturation"
    ctx.close()


def m3_problem(name):
    """M = 3 with a FREE interior time (node 1: the row H(X-) - H(X+)), a CONTINUOUS one and a FREE final time; rows on a trajectory,
    their costates moved by a few per cent."""
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    D = 1 if name == "osc1d_h" else 6
    S, M, N, tf = 2 * D, 3, 6, 1.8
    P = [4.0] if name == "osc1d_h" else cpu.DINT_P
    X0 = np.array([0.7, -0.4]) if name == "osc1d_h" else np.array(cpu.X0_DINT)
    nodes = [X0] + [np.array(hm.integrate(name, P, (0.0, 0.0), 0.0, k * tf / M, X0, N)[-1]) for k in (1, 2)]
    mode_x = np.zeros((M + 1, D), dtype=np.int32)
    mode_x[1:M] = CONTINUOUS
    mode_x[M, D // 2:] = FREE
    xn = np.zeros((M + 1, S))
    xn[0, :D] = X0[:D]
    xn[M, :D] = 0.3
    prob = Problem(D, [FIXED, FREE, CONTINUOUS, FREE], mode_x, np.array([0.0, 0.6, 1.2, 1.8]), xn)
    rng = np.random.default_rng(45)
    Z = np.tile(np.concatenate([np.concatenate(nodes), [0.55, 1.9]]), (3, 1))
    Z[1:] *= 1.0 + 0.03 * rng.uniform(-1.0, 1.0, size=(2, Z.shape[1]))
    if name == "dint_h":
        Z[2, 12 + 9:12 + 12] *= 8.0                                   # segment 1 of the last row saturates the control
    assert prob.n == Z.shape[1] == S * M + 2
    return P, prob, Z, N


@pytest.mark.parametrize("name", list(H_MODELS))
def test_h_only_residual_and_fd_jacobian_equal_the_restatement(name):
    P, prob, Z, N = m3_problem(name)
    ctx = context(name, P, N=N)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    F = ctx.residual_batch(Z)
    want = np.array([hm.residual_row(name, P, SW_CTX, prob, z, N) for z in Z])
    assert np.isfinite(want).all()
    assert np.array_equal(F.view(np.uint64), want.view(np.uint64)), "residual_batch, M = 3, free interior and final time"
    # MINPACK's forward differences (fdjac1), as tests/test_gpu_vtol.py restates them
    z0, n = Z[2], prob.n
    epsfcn = 1e-15
    eps = np.sqrt(max(epsfcn, np.finfo(float).eps))
    h = eps * np.abs(z0)
    h[h == 0] = eps
    Zp = np.tile(z0, (n, 1))
    Zp[np.arange(n), np.arange(n)] += h
    Fp = np.array([hm.residual_row(name, P, SW_CTX, prob, z, N) for z in Zp])
    J = ((Fp - want[2][None, :]) / h[:, None]).T
    for dedup in (False, True):
        got = ctx.fd_jacobian(z0, F[2], epsfcn=epsfcn, dedup=dedup)
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(J).view(np.uint64)), "fd_jacobian, dedup=%s" % dedup
    ctx.close()


@pytest.mark.parametrize("name", list(H_MODELS))
def test_h_only_trace_ends_where_integrate_batch_ends(name):
    from oracle.oracle import Problem, FIXED
    device, base, P, t, sw, X = H_MODELS[name]()
    B, N, T = 9, 20, 1.5
    X = np.ascontiguousarray(X[:B])
    D, S = X.shape[1] // 2, X.shape[1]
    ctx = context(device, P, N=N)
    prob = Problem(D, [FIXED, FIXED], np.zeros((2, D), dtype=np.int32), np.array([0.0, T]), np.zeros((2, S)))
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == S
    rows, count = ctx.trace_batch(X, stride=7)
    Xf = ctx.integrate_batch(0.0, T, X)
    last = np.array([rows[b, 0, count[b, 0] - 1] for b in range(B)])
    assert np.array_equal(np.ascontiguousarray(last[:, 1:1 + S]).view(np.uint64), Xf.view(np.uint64)), "the last trace row is the end state"
    dt, tk = (T - 0.0) / N, 0.0                                        # the loop's own time of the last row: t + h of the last step
    while tk + dt < (T - dt / 2):
        tk = tk + dt
    assert np.array_equal(last[:, 0], np.full(B, tk + ((T - tk) if tk + dt > T else dt)))
    H = np.array([hm.plain_hamiltonian(name, P, SW_CTX, T, Xf[b]) for b in range(B)])
    assert np.array_equal(np.ascontiguousarray(last[:, 1 + S + ctx.nu]).view(np.uint64), H.view(np.uint64)), "and its H is the plain Hamiltonian"
    ctx.close()


# ---- 4. end to end -----------------------------------------------------------------------------------------------------------------

def test_dint_h_solves_testDoubleIntegrator_like_the_in_tree_model():
    """testDoubleIntegrator's problem (M = 1, free tf, n = 13): hybrd from the same start converges with info = 1 for the model
    written from H alone, to within 1e-8 of the in-tree model's converged unknowns (the project's bar for converged solutions)."""
    c = jc.dint()
    prob, Z0 = c["prob"], np.ascontiguousarray(c["Z"][1:3])
    assert prob.n == 13 and prob.M == 1
    sol = {}
    for model in ("dint", "dint_h"):
        ctx = context(model, c["params"], N=c["N"])
        assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == 13
        sol[model] = ctx.multistart_solve(Z0, xtol=1e-10)
        ctx.close()
    gap = np.max(np.abs(sol["dint_h"]["z"] - sol["dint"]["z"]))
    print("dint_h against the in-tree double integrator, testDoubleIntegrator's problem: info %s / %s, nfev %s / %s, |z_h - z| = %.3e"
          % (sol["dint_h"]["info"].tolist(), sol["dint"]["info"].tolist(), sol["dint_h"]["nfev"].tolist(), sol["dint"]["nfev"].tolist(), gap))
    assert np.all(sol["dint"]["info"] == 1) and np.all(sol["dint_h"]["info"] == 1)
    assert gap <= 1e-8
