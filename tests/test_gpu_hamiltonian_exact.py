"""GPU: the Jacobian of the Hamiltonian vector field (socp_hamiltonian_jacobian_batch[_dev], capi.Context.hamiltonian_jacobian_batch)
and the exact entries of the models written from their Hamiltonian alone through SOCP_DEFINE_HAMILTONIAN_PLUGIN_EXACT
(tests/plugin/osc1d_hx_plugin.hip, dint_hx_plugin.hip) against tests/hamiltonian_exact_reference.py -- nested dual numbers restated in
Python.  Outputs live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions
of test_gpu_exact_jacobian.py); the run helpers are the neighbouring suites' own.  Every output is bit-equal to the restatement, in
both flavours.  A reference is computed once for a few distinct rows, which larger batches repeat.  The figures the tests print are
kept in profiles/hamiltonian_exact_gpu_tests.txt.  Without the feature the point call, the entries and the plugins do not exist."""
import numpy as np
import pytest

import exact_jacobian_reference as ejr
import fields_reference as fr
import hamiltonian_exact_reference as hx
import hamiltonian_model_reference as hm
import newton_cases as nc
import newton_reference as nr
import sensitivity_reference as sr
import test_gpu_exact_jacobian as xj
import test_gpu_fields_batch as fb
import test_gpu_hamiltonian_model as gm
import test_gpu_newton_batch as nb
import test_gpu_sensitivity_batch as sb
import test_hamiltonian_model_cpu as cpu
from test_gpu_jacobi_batch import SENT, GUARD, DP, sentinel, canon, plugin_path   # noqa: F401

pytestmark = pytest.mark.gpu
B_ALL = 130
SIZES = (1, 63, 64, 65, 130)
PLUGIN_IDS = {"lqr1d": 1001, "osc1d_exact_jacobian": 1005, "osc1d_h": 1008, "dint_h": 1009, "osc1d_hx": 1010, "dint_hx": 1011}
SW_CTX = gm.SW_CTX
VARIANTS = ("exact", "fast")
N = 20


def context(model, params, variant="exact", steps=N, prob=None):
    from socp_amd import capi
    if model in PLUGIN_IDS:
        capi.plugin_load(plugin_path(model))
        ctx = capi.Context(PLUGIN_IDS[model], nparams=len(params))
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[model])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(np.asarray(params, dtype=np.float64))
    ctx.set_step_number(steps)
    if prob is None:
        ctx.set_switching_times(SW_CTX)
    else:
        assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


# ---- 1. the point call ---------------------------------------------------------------------------------------------------------------

POINTS = dict(gm.POINTS)
POINTS.update({"osc1d_hx": lambda: gm.osc1d_points("osc1d_hx"), "dint_hx": lambda: gm.dint_points("dint_hx")})
_POINTS, _REF = {}, {}


def points(name):
    if name not in _POINTS:
        _POINTS[name] = POINTS[name]()
    return _POINTS[name]


def reference(name):
    """(A[130][S * S] column-major, G[130][S]) of the restatement, computed once."""
    if name not in _REF:
        device, model, P, t, sw, X = points(name)
        A, G = hx.hamiltonian_jacobian_batch(model, P, t, X, sw=sw, sw_default=SW_CTX)
        assert np.all(np.isfinite(A)) and np.all(np.isfinite(G))
        A.setflags(write=False)
        G.setflags(write=False)
        _REF[name] = (A, G)
    return _REF[name]


def run_host(ctx, t, sw, X, g=True):
    t, X = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64)
    sw = np.ascontiguousarray(sw, dtype=np.float64) if sw is not None else None
    S = X.shape[1]
    A, G = sentinel(X.size * S), sentinel(X.size)
    ctx._chk(ctx.L.socp_hamiltonian_jacobian_batch(ctx.h, len(X), t.ctypes.data_as(DP), sw.ctypes.data_as(DP) if sw is not None else None,
                                                   X.ctypes.data_as(DP), A.ctypes.data_as(DP), G.ctypes.data_as(DP) if g else None))
    return A.view(np.uint64), G.view(np.uint64)


def run_dev(ctx, t, sw, X, g=True):
    import torch
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()                 # noqa: E731
    X = np.asarray(X)
    dt, dX, dsw = up(t), up(X), (up(sw) if sw is not None else None)
    dA, dG = torch.from_numpy(sentinel(X.size * X.shape[1])).cuda(), torch.from_numpy(sentinel(X.size)).cuda()
    torch.cuda.synchronize()
    ctx.hamiltonian_jacobian_batch_dev(len(X), dt.data_ptr(), dsw.data_ptr() if dsw is not None else None, dX.data_ptr(), dA.data_ptr(),
                                       dG.data_ptr() if g else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return dA.cpu().numpy().view(np.uint64), dG.cpu().numpy().view(np.uint64)


def check_whole(got, want, what):
    for label, g, w in zip(("A", "G"), got, want):
        if w is None:
            assert np.all(g == np.uint64(SENT)), "%s: %s was written although its pointer was NULL" % (what, label)
            continue
        w = np.ascontiguousarray(w, dtype=np.float64).ravel().view(np.uint64)
        assert g.size == w.size + GUARD
        assert np.all(g[w.size:] == np.uint64(SENT)), "%s: guard words behind %s were written" % (what, label)
        gg, ww = canon(g[:w.size]), canon(w)
        bad = np.argwhere(gg != ww).ravel()
        assert len(bad) == 0, (what, label, "%d differ; first flat indices:" % len(bad), bad[:5].tolist(), gg[bad[:5]].view(np.float64),
                               ww[bad[:5]].view(np.float64))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(POINTS))
def test_point_call_equals_the_restatement(name, variant):
    device, model, P, t, sw, X = points(name)
    A, G = reference(name)
    ctx = context(device, P, variant)
    assert ctx.has_hamiltonian_jacobian() and ctx.L.socp_ctx_has_hamiltonian_jacobian(ctx.h) == 1
    t0, l0 = ctx.counters()
    for B in SIZES:
        cut = (t[:B], sw[:B] if sw is not None else None, X[:B])
        # the first B rows of the batch of 130: bit-equal to those rows of the whole batch
        check_whole(run_host(ctx, *cut), (A[:B], G[:B]), "%s, B = %d, host form" % (name, B))
        check_whole(run_dev(ctx, *cut), (A[:B], G[:B]), "%s, B = %d, _dev form" % (name, B))
    check_whole(run_dev(ctx, t[:65], sw[:65] if sw is not None else None, X[:65], g=False), (A[:65], None), name + ", d_G = NULL")
    check_whole(run_host(ctx, t[:65], sw[:65] if sw is not None else None, X[:65], g=False), (A[:65], None), name + ", G = NULL, host form")
    t1, l1 = ctx.counters()
    assert (t1 - t0, l1 - l0) == (0, 2 * len(SIZES) + 2), "one launch per call, no trajectory"
    Ap, Gp = ctx.hamiltonian_jacobian_batch(t, X, sw=sw, gradient=True)
    S = X.shape[1]
    assert np.array_equal(canon(np.ascontiguousarray(Ap.transpose(0, 2, 1)).reshape(len(X), S * S).view(np.uint64)), canon(A.view(np.uint64))), "the binding"
    grad = ctx.hamiltonian_gradient_batch(t, X, sw=sw)
    assert np.array_equal(Gp.view(np.uint64), grad.view(np.uint64)), "G is socp_hamiltonian_gradient_batch, bit for bit"
    assert np.array_equal(grad.view(np.uint64), hm.gradient_batch(model, P, t, X, sw=sw, sw_default=SW_CTX).view(np.uint64))
    D = S // 2
    Hs = np.concatenate([-Ap[:, D:, :], Ap[:, :D, :]], axis=1)                             # -Omega A
    asym = np.max(np.abs(Hs - Hs.transpose(0, 2, 1)), axis=(1, 2)) / np.maximum(1.0, np.max(np.abs(Ap), axis=(1, 2)))
    print("%-28s %-5s max |(-Omega A) - (-Omega A)^T| / max(1, |A|) over 130 points = %.3e" % (name, variant, asym.max()))
    if name.startswith("goddard general"):
        s0, s1 = (sw[:, 0], sw[:, 1]) if sw is not None else SW_CTX
        arc = np.where(t <= s0, 0, np.where(t <= s1, 1, 2))
        assert {0, 1, 2} == set(arc.tolist()), "all three arcs of the general law"
    if model == "covid":
        u = (X[:, 5] - X[:, 4]) * X[:, 0] * X[:, 2] / P[1] / P[3] * P[0]
        combos = {(bool(a <= P[6]), bool(a >= P[7]), bool(i >= P[4])) for a, i in zip(u, X[:, 2])}
        assert len(combos) == 6, "every clamp / penalty combination"
    ctx.close()


def test_goddard_takes_the_law_from_the_contexts_mu2():
    assert not np.array_equal(reference("goddard smooth")[0], reference("goddard general, context sw")[0])


def test_models_without_the_entry_are_refused():
    import torch
    from socp_amd import capi
    gold = np.load(gm.jc.os.path.join(gm.jc.ROOT, "tests", "golden", "vtol_vectors.npz"))
    others = [("interceptor", capi.Context(capi.MODEL_INTERCEPTOR))]
    cv = capi.Context(capi.MODEL_VTOLUAV)
    cv.set_map(gold["table_shipped"])
    others.append(("vtolUAV", cv))
    capi.plugin_load(plugin_path("lqr1d"))
    others.append(("lqr1d plugin", capi.Context(PLUGIN_IDS["lqr1d"], nparams=1)))
    fresh = lambda a: bool(np.all(a.view(np.uint64) == np.uint64(SENT)))                   # noqa: E731
    for label, cx in others:
        S = cx.s
        assert not cx.has_hamiltonian_jacobian() and cx.L.socp_ctx_has_hamiltonian_jacobian(cx.h) == 0, label
        Xo, to, ao, go = np.full((3, S), 0.5), np.zeros(3), sentinel(3 * S * S), sentinel(3 * S)
        dXo, dto, dao = torch.from_numpy(Xo).cuda(), torch.from_numpy(to).cuda(), torch.from_numpy(sentinel(3 * S * S)).cuda()
        torch.cuda.synchronize()
        c0 = cx.counters()
        assert cx.L.socp_hamiltonian_jacobian_batch(cx.h, 3, to.ctypes.data_as(DP), None, Xo.ctypes.data_as(DP), ao.ctypes.data_as(DP),
                                                    go.ctypes.data_as(DP)) == capi.ERR_UNSUPPORTED
        assert "no hamiltonian_jacobian entry" in cx.L.socp_last_error(cx.h).decode(), label
        assert cx.L.socp_hamiltonian_jacobian_batch_dev(cx.h, 3, dto.data_ptr(), None, dXo.data_ptr(), dao.data_ptr(), None) == capi.ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert cx.counters() == c0 and fresh(ao) and fresh(go) and fresh(dao.cpu().numpy()), label
        with pytest.raises(capi.SocpError) as e:
            cx.hamiltonian_jacobian_batch(to, Xo)
        assert e.value.code == capi.ERR_UNSUPPORTED
        cx.close()
    ctx = context("dint", cpu.DINT_P)
    L, h = ctx.L, ctx.h
    assert L.socp_hamiltonian_jacobian_batch(h, -1, None, None, None, None, None) == capi.ERR_ARG and "B >= 0" in L.socp_last_error(h).decode()
    assert L.socp_hamiltonian_jacobian_batch(h, 0, None, None, None, None, None) == capi.OK
    assert L.socp_hamiltonian_jacobian_batch_dev(h, 0, None, None, None, None, None) == capi.OK
    assert L.socp_hamiltonian_jacobian_batch(None, 1, None, None, None, None, None) == capi.ERR_ARG
    assert L.socp_ctx_has_hamiltonian_jacobian(None) == capi.ERR_ARG
    ctx.close()


# ---- 2. the new entries on the exact plugins -------------------------------------------------------------------------------------------

def test_exact_plugins_have_the_entries_and_the_plain_ones_do_not():
    for model, P, want in (("osc1d_hx", [4.0], True), ("dint_hx", cpu.DINT_P, True), ("osc1d_h", [4.0], False), ("dint_h", cpu.DINT_P, False)):
        ctx = context(model, P)
        assert (ctx.has_fields(), ctx.has_exact_jacobian(), ctx.has_sensitivity()) == (want, want, want), model
        assert [ctx.L.socp_ctx_has_fields(ctx.h), ctx.L.socp_ctx_has_exact_jacobian(ctx.h), ctx.L.socp_ctx_has_sensitivity(ctx.h)] == [int(want)] * 3, model
        assert ctx.has_hamiltonian_gradient() and ctx.has_hamiltonian_jacobian(), "every hamiltonian_t here takes nested numbers"
        ctx.close()


# ---- the shooting problems of the exact plugins: a few distinct rows, repeated to fill a batch ----------------------------------------

def problem(model, kind):
    """(P, prob, rows[R][n]): kind "m1"; "m3free" -- M = 3, a FREE interior time (node 1: the row H(X-) - H(X+) and its -grad H(X+)
    part), a CONTINUOUS one and a FREE final time; "m3fixed" -- M = 3, node 1 a FIXED interior state, fixed times.  For dint_hx one
    row has a saturated segment."""
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    base = hx.BASE[model]
    D = 1 if base == "osc1d" else 6
    S, tf = 2 * D, 1.8
    P = [4.0] if base == "osc1d" else cpu.DINT_P
    X0 = np.array([0.7, -0.4]) if base == "osc1d" else np.array(cpu.X0_DINT)
    rng = np.random.default_rng(46)
    if kind == "m1":
        mode_x = np.zeros((2, D), dtype=np.int32)
        mode_x[1, D // 2:] = FREE
        xn = np.zeros((2, S))
        xn[0, :D] = X0[:D]
        xn[1, :D] = 0.3
        prob = Problem(D, [FIXED, FIXED], mode_x, np.array([0.0, tf]), xn)
        rows = np.tile(X0, (3, 1))
    else:
        M = 3
        nodes = [X0] + [np.array(hm.integrate(base, P, (0.0, 0.0), 0.0, k * tf / M, X0, N)[-1]) for k in (1, 2)]
        mode_x = np.zeros((M + 1, D), dtype=np.int32)
        mode_x[1:M] = CONTINUOUS
        mode_x[M, D // 2:] = FREE
        xn = np.zeros((M + 1, S))
        xn[0, :D] = X0[:D]
        xn[M, :D] = 0.3
        if kind == "m3free":
            prob = Problem(D, [FIXED, FREE, CONTINUOUS, FREE], mode_x, np.array([0.0, 0.6, 1.2, 1.8]), xn)
            rows = np.tile(np.concatenate([np.concatenate(nodes), [0.55, 1.9]]), (3, 1))
        else:
            mode_x[1] = FIXED
            xn[1, :D] = nodes[1][:D] * 1.01
            prob = Problem(D, [FIXED, FIXED, FIXED, FIXED], mode_x, np.array([0.0, 0.6, 1.2, 1.8]), xn)
            rows = np.tile(np.concatenate(nodes), (3, 1))
    rows[1:] *= 1.0 + 0.03 * rng.uniform(-1.0, 1.0, size=rows[1:].shape)
    if base == "dint":
        first = 0 if kind == "m1" else 12
        rows[2, first + 9:first + 12] *= 8.0                            # the control saturates on that segment
    assert prob.n == rows.shape[1]
    return P, prob, rows


def node_times(prob, z):
    """Timeline::nt of exact_jacobian_reference in doubles: FIXED from the problem, FREE from z, the others interpolated."""
    lay = ejr.Layout(prob)
    jt = lambda j: float(z[lay.kind[j]]) if lay.kind[j] >= 0 else float(prob.time[j])     # noqa: E731
    out = []
    for k in range(prob.M + 1):
        if lay.kind[k] >= -1:
            out.append(jt(k))
        else:
            a, b = lay.lo[k], lay.hi[k]
            ta, tb = jt(a), jt(b)
            out.append(ta + (k - a) * (tb - ta) / (b - a))
    return out


def tiled(rows, B):
    return np.ascontiguousarray(rows[np.arange(B) % len(rows)])


_XJ = {}


def exact_jacobian_reference(model, kind, blocks=None):
    """(Fjac[R][n * n] column-major, F[R][n]) of the distinct rows (with blocks: of the distinct (row, block) pairs)."""
    key = (model, kind, blocks is not None)
    if key not in _XJ:
        P, prob, rows = problem(model, kind)
        with hx.entries():
            _XJ[key] = ejr.exact_jacobian_batch(model, [float(p) for p in P], (0.0, 0.0), prob, rows, N, blocks=blocks)
    return _XJ[key]


# ---- 3. fields -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["m1", "m3free"])
def test_fields_of_dint_hx_equal_the_restatement(kind):
    P, prob, rows = problem("dint_hx", kind)
    B, stride, cap = 65, 5, 8
    c = dict(model="dint_hx", prob=prob, params=P, N=N)
    with hx.entries():
        slabs = []
        for z in rows:
            tl = node_times(prob, z)
            slabs.append([fr.fields_segment("dint_hx", P, (0.0, 0.0), 6, float(tl[i]), float(tl[i + 1]), z[12 * i:12 * (i + 1)], N, cols=fr.ALL,
                                            stride=stride, skip=0) for i in range(prob.M)])
    slabs = [slabs[b % len(rows)] for b in range(B)]
    Z = tiled(rows, B)
    for variant in VARIANTS:
        ctx = context("dint_hx", P, variant, prob=prob)
        assert ctx.has_fields()
        for cols in (fr.COSTATE, fr.ALL):
            want = fb.expected(c, slabs, cols, skip=0, cap=cap)
            fb.check_whole(fb.run_host(ctx, Z, cols, stride=stride, skip=0, cap=cap), want, "dint_hx %s cols = %d, host form, %s" % (kind, cols, variant))
            fb.check_whole(fb.run_dev(ctx, Z, cols, stride=stride, skip=0, cap=cap), want, "dint_hx %s cols = %d, _dev form, %s" % (kind, cols, variant))
        ctx.close()


# ---- 4. the exact Jacobian -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["m1", "m3free", "m3fixed"])
@pytest.mark.parametrize("model", ["dint_hx", "osc1d_hx"])
def test_exact_jacobian_equals_the_restatement(model, kind):
    P, prob, rows = problem(model, kind)
    J, F = exact_jacobian_reference(model, kind)
    R, n, S = len(rows), prob.n, 2 * prob.dim
    pick = lambda B: np.arange(B) % R                                                    # noqa: E731
    # per-row blocks: the first parameter and the desired final state move with the row (R distinct blocks, repeated like the rows)
    params = np.tile(np.concatenate([P, [0.0, 0.0]]), (R, 1))
    params[:, 0] *= np.linspace(1.0, 1.2, R)
    xnode = np.tile(prob.xnode.ravel(), (R, 1))
    xnode[:, prob.M * S] += np.linspace(0.0, 0.05, R)
    Jb, Fb = exact_jacobian_reference(model, kind, blocks=(params, None, xnode))
    for variant in VARIANTS:
        ctx = context(model, P, variant, prob=prob)
        assert ctx.has_exact_jacobian()
        for B in (1, 64, 65, 70):
            Z = tiled(rows, B)
            xj.check_whole(xj.run_dev(ctx, Z), (J[pick(B)], F[pick(B)]), "%s %s B = %d, _dev form, %s" % (model, kind, B, variant))
        Z = tiled(rows, 70)
        xj.check_whole(xj.run_host(ctx, Z), (J[pick(70)], F[pick(70)]), "%s %s B = 70, host form, %s" % (model, kind, variant))
        xj.check_whole(xj.run_host(ctx, Z, blocks=(params[pick(70)], None, xnode[pick(70)])), (Jb[pick(70)], Fb[pick(70)]),
                       "%s %s B = 70, _blocks form, %s" % (model, kind, variant))
        # F is socp_residual_batch on the same context: the value parts are the plain right-hand side's
        Fr = ctx.residual_batch(tiled(rows, 65))
        assert np.array_equal(canon(Fr.view(np.uint64)), canon(np.ascontiguousarray(F[pick(65)]).view(np.uint64))), "F against socp_residual_batch"
        if prob.M > 1:
            Jm = xj.matrices(xj.run_dev(ctx, tiled(rows, R))[0], R, n)
            phi = ctx.fields_batch(tiled(rows, R), cols=fr.ALL, stride=N, cap=4, phi=True)["phi"].cpu().numpy()
            D = prob.dim
            for i in range(prob.M - 1):
                # the rows X - Xp (or X - xd) of node i + 1 are Phi's; the second row of a FIXED component reads Xp alone
                block = Jm[:, S * (i + 1):S * (i + 2), S * i:S * (i + 1)]
                free = [j for j in range(D) if prob.mode_x[i + 1][j] != 0]
                fixed = [j for j in range(D) if prob.mode_x[i + 1][j] == 0]
                keep = list(range(D)) + [D + j for j in free]
                assert np.array_equal(block[:, keep], phi[:, i][:, keep]), "the continuity blocks are Phi"
                assert not np.any(block[:, [D + j for j in fixed]]), "Xp - xd does not depend on the arriving segment"
        ctx.close()


# ---- 5. sensitivities ----------------------------------------------------------------------------------------------------------------------

def test_sensitivities_of_dint_hx_equal_the_restatement():
    P, prob, rows = problem("dint_hx", "m3free")
    S = 12
    dirs = [(sr.DIR_PARAM, 0), (sr.DIR_PARAM, 1), (sr.DIR_PARAM, 2), (sr.DIR_TIME, 0), (sr.DIR_XNODE, 3 * S + 1)]
    B = 65
    Z = tiled(rows, B)
    with hx.entries():
        r = sr.sensitivity_batch("dint_hx", [float(p) for p in P], (0.0, 0.0), prob, Z, N, dirs)
    want = (r["dz"], r["info"], r["g"])
    u = -rows[2, 12 + 9:12 + 12] / P[1]
    assert np.sqrt(u @ u) > P[0] and np.abs(r["g"][2, 0]).max() > 0, "a saturated segment among the rows: u_max matters"
    assert np.all(r["info"] == 0) and np.isfinite(r["dz"]).all()
    for variant in VARIANTS:
        ctx = context("dint_hx", P, variant, prob=prob)
        assert ctx.has_sensitivity()
        sb.check_whole(sb.run_host(ctx, Z, dirs), want, "dint_hx sensitivities, host form, " + variant)
        sb.check_whole(sb.run_dev(ctx, Z, dirs), want, "dint_hx sensitivities, _dev form, " + variant)
        ctx.close()


# ---- 6. the Newton polish ------------------------------------------------------------------------------------------------------------------

def test_newton_polish_of_dint_hx_on_testDoubleIntegrator():
    """testDoubleIntegrator's problem (M = 1, free tf, n = 13, N = 50) from starts 1e-4 off the in-tree model's stored solution: every
    row ends CONVERGED within 1e-8 of that solution, all outputs bit-equal to newton_reference fed with the restated exact Jacobian."""
    c = nc.dint()
    Z = np.stack([nc.perturbed(c["root"], 1e-4, s) for s in (1, 2)])
    kw = dict(jac=2, ftol=1e-11, trials=4, rounds=6)
    own = np.concatenate([np.asarray(c["params"], dtype=np.float64), [0.0, 0.0]])
    with hx.entries():
        ref = nr.newton_reference("dint_hx", None, c["prob"], 3, c["N"], Z, nr.options(**kw), own=own)
    print("dint_hx newton: status %s iters %s nhalf %s rnorm %s |z - z_dint| = %.3e"
          % (ref["status"], ref["iters"], ref["nhalf"], ref["rnorm"], np.max(np.abs(ref["z"] - c["root"][None]))))
    assert np.all(ref["status"] == nr.CONVERGED)
    assert np.max(np.abs(ref["z"] - c["root"][None])) <= 1e-8
    from socp_amd import capi
    for variant in VARIANTS:
        ctx = context("dint_hx", c["params"], variant, steps=c["N"], prob=c["prob"])
        dopts = capi.newton_options(**kw)
        got = nb.run_dev(ctx, Z, dopts)
        nb.check_whole(got, ref, "dint_hx newton, _dev form, " + variant)
        nb.check_whole(nb.run_host(ctx, Z, dopts), ref, "dint_hx newton, host form, " + variant)
        zout = got["z"][:Z.size].view(np.float64).reshape(Z.shape)
        assert np.max(np.abs(zout - c["root"][None])) <= 1e-8, "within 1e-8 of the in-tree model's solution"
        ctx.close()
