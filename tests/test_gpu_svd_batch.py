"""GPU: socp_svd_batch_dev and socp_singular_batch[_dev] / _blocks (capi.Context.svd_batch_dev, singular_batch) against
tests/svd_reference.py -- the definition of include/socp_hip.h restated in numpy.  Outputs live in sentinel-filled buffers followed
by 64 guard words and are compared WHOLE on integer views (the conventions of test_gpu_tangent_batch.py).
Reference-order flavour: sigma, Vt, sweeps and info bit-equal to the restatement (a NaN equals any NaN).  Throughput flavour: the
same info and the three bounds of test_svd_cpu.py against LAPACK with the same c = svd_reference.C_BOUND.
The shapes are the smallest at which the team packing (n = 14 .. 16, B = 37: eight matrices per workgroup and a partial last one),
the phantom row (odd n), the wave boundary (n = 64 / 65 lanes; 127; two wavefronts per matrix above 128) and the large-LDS path
(n >= 65: more than 64 KiB; n = 142: all of it) can each go wrong."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import events_cases as ec
import svd_reference as sr
import tangent_reference as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGIN = os.path.join(ROOT, "socp_amd", "_build", "plugins", "liblqr1d_plugin.so")
SENT = 0x7FF8DEADBEEF0001                       # a NaN no kernel produces
SENT_I = 0x5EADBEE1
GUARD = 64
N_MAX = 142
SHAPES = [(1, 5), (2, 5), (3, 5), (14, 37), (15, 37), (16, 37), (64, 5), (65, 5), (85, 9), (127, 3), (N_MAX, 2)]
CB = sr.C_BOUND


def sentinel(size):
    return np.full(size + GUARD, np.uint64(SENT), dtype=np.uint64).view(np.float64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def same_doubles(got, want):
    """Bit equality, a NaN equal to any NaN."""
    g, w = got.view(np.float64), np.ascontiguousarray(want, dtype=np.float64).ravel()
    return (got == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))


def svd_context(variant="exact"):
    from socp_amd import capi
    ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)          # no problem is set: the call is model-independent
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    return ctx


def run_svd(ctx, A, max_sweeps=sr.MAX_SWEEPS, vt=True):
    """The call on guarded device buffers: the WHOLE buffers (sigma, Vt, sweeps, info) back, doubles as integer views.  A sits in a
    guarded buffer too and must come back as it went in; exactly one launch is counted."""
    import torch
    A = np.ascontiguousarray(A, dtype=np.float64)
    B, nn = A.shape
    n = int(round(np.sqrt(nn)))
    host_A = np.concatenate([A.ravel(), sentinel(0)])
    dA, dS, dV, dW, dI = up(host_A), up(sentinel(B * n)), up(sentinel(B * nn)), up(sentinel_i(B)), up(sentinel_i(B))
    torch.cuda.synchronize()
    launches = ctx.counters()[1]
    ctx.svd_batch_dev(B, n, dA.data_ptr(), max_sweeps, dS.data_ptr(), dV.data_ptr() if vt else None, dW.data_ptr(), dI.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert ctx.counters()[1] == launches + 1, "one launch"
    assert np.array_equal(dA.cpu().numpy().view(np.uint64), host_A.view(np.uint64)), "A (or the guard words behind it) was written"
    return dS.cpu().numpy().view(np.uint64), dV.cpu().numpy().view(np.uint64), dW.cpu().numpy(), dI.cpu().numpy()


def check_whole(got, ref, B, n, what, vt=True):
    sigma, Vt, sweeps, info = got
    assert np.all(sigma[B * n:] == np.uint64(SENT)) and np.all(sweeps[B:] == SENT_I) and np.all(info[B:] == SENT_I), what + ": guard words"
    if vt:
        assert np.all(Vt[B * n * n:] == np.uint64(SENT)), what + ": guard words behind Vt"
    else:
        assert np.all(Vt == np.uint64(SENT)), what + ": Vt was written although its pointer was NULL"
    assert np.array_equal(info[:B], ref["info"]), (what, "info", info[:B], ref["info"])
    assert np.array_equal(sweeps[:B], ref["sweeps"]), (what, "sweeps", sweeps[:B], ref["sweeps"])
    for name, g, w in (("sigma", sigma[:B * n], ref["sigma"]),) + ((("Vt", Vt[:B * n * n], ref["vt"]),) if vt else ()):
        bad = np.argwhere(~same_doubles(g, w)).ravel()
        assert len(bad) == 0, (what, name, "%d differ, first flat indices:" % len(bad), bad[:5].tolist(), g.view(np.float64)[bad[:5]],
                               np.ravel(w)[bad[:5]])


def batch(n, B):
    """(A[B][n*n], the restatement's result): the graded matrices where the CPU test has them, an identity, the zero matrix (from
    n = 14 on, B allowing), random matrices for the rest; n = 14: the mixed batch of svd_reference too.  Computed once."""
    def build():
        parts = []
        if n in sr.SIZES:
            parts.append(sr.graded_reference(n)[0])
        if n == 14:
            parts.append(sr.mixed_batch(n))
        if B >= 9:
            parts += [np.eye(n).reshape(1, -1), np.zeros((1, n * n))]
        have = sum(len(p) for p in parts)
        if have < B:
            parts.append(sr.random_batch(n, B - have))
        A = np.concatenate(parts)[:B]
        A.setflags(write=False)
        return A, sr.svd_batch(A, sr.MAX_SWEEPS)
    return sr.cached(("gpu", n, B), build)


# ---- 1. reference-order flavour, bit for bit ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n,B", SHAPES)
def test_svd_reference_order_bit_for_bit(n, B):
    A, ref = batch(n, B)
    assert len(A) == B
    expect_bad = 2 if n == 14 else 0
    assert int(np.sum(ref["info"] == 2)) == expect_bad and int(np.sum(ref["info"] == 1)) == 0
    ctx = svd_context()
    check_whole(run_svd(ctx, A), ref, B, n, "n = %d" % n)
    if n in (3, 16, 65, N_MAX):
        check_whole(run_svd(ctx, A, vt=False), ref, B, n, "n = %d, NULL Vt" % n, vt=False)
    ctx.close()


def test_svd_corner_cases_against_hand_written_answers():
    """The corner cases of test_svd_cpu.py on the device, both flavours (no rotation happens, so the flavours agree bit for bit):
    n = 1 (the vector is +1 whatever the entry's sign, 0 for a zero), identities, a permuted diagonal with signs and a tie."""
    for variant in ("exact", "fast"):
        ctx = svd_context(variant)
        sigma, Vt, sweeps, info = run_svd(ctx, np.array([[-2.5], [0.0], [3.0]]))
        assert np.array_equal(sigma[:3].view(np.float64), [2.5, 0.0, 3.0]) and np.array_equal(Vt[:3].view(np.float64), [1.0, 0.0, 1.0])
        assert np.array_equal(sweeps[:3], [1, 1, 1]) and np.array_equal(info[:3], [0, 0, 0])
        for n in (2, 5, 14):
            sigma, Vt, sweeps, info = run_svd(ctx, np.eye(n).reshape(1, -1))
            assert sweeps[0] == 1 and info[0] == 0 and np.array_equal(sigma[:n].view(np.float64), np.ones(n))
            assert np.array_equal(Vt[:n * n].view(np.float64), np.eye(n).ravel())
        A, want_sigma, want_Vt = sr.permuted_diagonal()
        sigma, Vt, sweeps, info = run_svd(ctx, A)
        assert sweeps[0] == 1 and info[0] == 0 and np.array_equal(sigma[:5].view(np.float64), want_sigma)
        assert np.array_equal(Vt[:25].view(np.float64), want_Vt.ravel())
        ctx.close()


def test_svd_mixed_fates_in_one_workgroup():
    """max_sweeps = 2, n = 14, eight matrices of one workgroup: an identity and the zero matrix finish in sweep 1, a NaN matrix never
    starts (info 2), the random ones are cut off (info 1, sweeps 2) -- each between neighbours of another fate."""
    n = 14
    R = sr.random_batch(n, 4, seed=99)
    bad = R[1].copy()
    bad[17] = np.nan
    A = np.stack([R[0], np.eye(n).ravel(), bad, R[2], np.zeros(n * n), R[3], np.eye(n).ravel()[::-1].copy(), R[1]])
    ref = sr.svd_batch(A, 2)
    assert np.array_equal(ref["info"], [1, 0, 2, 1, 0, 1, 0, 1]) and np.array_equal(ref["sweeps"], [2, 1, 0, 2, 1, 2, 1, 2])
    for variant in ("exact", "fast"):
        ctx = svd_context(variant)
        got = run_svd(ctx, A, max_sweeps=2)
        if variant == "exact":
            check_whole(got, ref, 8, n, "mixed fates")
        else:
            assert np.array_equal(got[3][:8], ref["info"]) and np.array_equal(got[2][:8], ref["sweeps"])
        ctx.close()


# ---- 2. throughput flavour: the same info, the three bounds ---------------------------------------------------------------------

@pytest.mark.parametrize("n,B", SHAPES)
def test_svd_fast_flavour_info_and_bounds(n, B):
    A, ref = batch(n, B)
    ctx = svd_context("fast")
    sigma, Vt, sweeps, info = run_svd(ctx, A)
    ctx.close()
    assert np.all(sigma[B * n:] == np.uint64(SENT)) and np.all(Vt[B * n * n:] == np.uint64(SENT)) and np.all(sweeps[B:] == SENT_I) and np.all(info[B:] == SENT_I)
    assert np.array_equal(info[:B], ref["info"]), "info is the reference-order flavour's"
    sigma, Vt = sigma[:B * n].view(np.float64).reshape(B, n), Vt[:B * n * n].view(np.float64).reshape(B, n, n)
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        if info[b] == 2:
            assert np.all(np.isnan(sigma[b])) and np.all(np.isnan(Vt[b])) and sweeps[b] == 0
            continue
        assert 1 <= sweeps[b] <= sr.MAX_SWEEPS and np.all(np.diff(sigma[b]) <= 0)
        if not np.any(A[b]):
            assert np.all(sigma[b] == 0) and np.all(Vt[b] == 0)
            continue
        q = sr.accuracy_ratios(A[b], sigma[b], Vt[b, n - 1])
        worst = [max(a, c) for a, c in zip(worst, q)]
        assert max(q) <= CB, (n, b, q)
    print("fast n = %d: largest ratios sigma %.3f, |A vmin| %.3f, |vmin| %.3f (bound %g)" % (n, worst[0], worst[1], worst[2], CB))


# ---- 3. a row's result does not depend on how rows are batched --------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_svd_rows_alone_equal_rows_inside_the_batch(variant):
    ctx = svd_context(variant)
    for n, B, rows in ((14, 37, (0, 7, 13, 36)), (15, 37, (35,)), (85, 9, (1, 8))):
        A, _ = batch(n, B)
        whole = run_svd(ctx, A)
        for b in rows:
            alone = run_svd(ctx, A[b:b + 1])
            assert np.array_equal(alone[0][:n], whole[0][b * n:(b + 1) * n]), (variant, n, b, "sigma")
            assert np.array_equal(alone[1][:n * n], whole[1][b * n * n:(b + 1) * n * n]), (variant, n, b, "Vt")
            assert alone[2][0] == whole[2][b] and alone[3][0] == whole[3][b]
        pair = run_svd(ctx, A[[rows[-1], rows[0]]])                # another order, another team
        assert np.array_equal(pair[0][:n], whole[0][rows[-1] * n:(rows[-1] + 1) * n]) and np.array_equal(pair[0][n:2 * n], whole[0][rows[0] * n:(rows[0] + 1) * n])
    ctx.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------

def test_svd_refusals_write_nothing_and_launch_nothing():
    import torch
    from socp_amd import capi
    ctx = svd_context()
    L, h = ctx.L, ctx.h
    n, B = 5, 2
    A = sr.random_batch(n, B)
    dA, dS, dV, dW, dI = up(A), up(sentinel(B * n)), up(sentinel(B * n * n)), up(sentinel_i(B)), up(sentinel_i(B))
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    before = ctx.counters()

    def call(B_=B, n_=n, A_=p(dA), sweeps_=60, S_=p(dS), V_=p(dV), W_=p(dW), I_=p(dI)):
        return L.socp_svd_batch_dev(h, B_, n_, A_, sweeps_, S_, V_, W_, I_)
    assert call(B_=-1) == capi.ERR_ARG and call(n_=0) == capi.ERR_ARG and call(n_=-3) == capi.ERR_ARG
    assert call(sweeps_=0) == capi.ERR_ARG and call(sweeps_=1001) == capi.ERR_ARG and call(sweeps_=-1) == capi.ERR_ARG
    assert call(A_=None) == capi.ERR_ARG and call(S_=None) == capi.ERR_ARG and call(W_=None) == capi.ERR_ARG and call(I_=None) == capi.ERR_ARG
    assert call(n_=N_MAX + 1) == capi.ERR_UNSUPPORTED and "160 KiB" in L.socp_last_error(h).decode()
    assert call(n_=253) == capi.ERR_UNSUPPORTED and call(n_=832) == capi.ERR_UNSUPPORTED
    # B == 0: SOCP_OK, no launch, NULL pointers allowed
    assert call(B_=0) == capi.OK and L.socp_svd_batch_dev(h, 0, n, None, 60, None, None, None, None) == capi.OK
    ctx.synchronize()
    torch.cuda.synchronize()
    assert ctx.counters() == before, "the refused calls and B == 0 launched and counted nothing"
    for t, fill in ((dS, np.uint64(SENT)), (dV, np.uint64(SENT))):
        assert np.all(t.cpu().numpy().view(np.uint64) == fill), "a refused call wrote"
    assert np.all(dW.cpu().numpy() == SENT_I) and np.all(dI.cpu().numpy() == SENT_I)
    assert np.array_equal(dA.cpu().numpy(), A)
    # the limits themselves are accepted
    assert call(sweeps_=1) == capi.OK and call(sweeps_=1000) == capi.OK
    ctx.synchronize()
    assert ctx.counters()[1] == before[1] + 2
    ctx.close()


# ---- 5. socp_singular_batch on the models ---------------------------------------------------------------------------------------

def model_case(name):
    """dict(make = a function returning a fresh context with the problem set, Z[B][n], jac)."""
    def build():
        from socp_amd import capi
        if name == "goddard14":
            from conftest import goddard_single_problem
            prob, z = goddard_single_problem()

            def make(variant):
                ctx = capi.Context(capi.MODEL_GODDARD)
                ctx.set_param("mu2", 1.0)
                ctx.set_step_number(100)
                return ctx, prob
            return dict(make=make, Z=ec.perturbed(z, 5, 1e-3, seed=11), jac=0, n=14)
        if name == "goddard85":
            g = tr.goddard_case()

            def make(variant):
                ctx = capi.Context(capi.MODEL_GODDARD)
                ctx.set_params(g["params"])
                ctx.set_step_number(8)
                return ctx, g["prob"]
            return dict(make=make, Z=ec.perturbed(ec.goddard_stage3_row(), 3, 1e-3, seed=12), jac=0, n=85)
        if name in ("dint_fd", "dint_var"):
            d = tr.dint_case()

            def make(variant):
                ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)
                ctx.set_params(d["params"])
                ctx.set_step_number(d["N"])
                return ctx, d["prob"]
            return dict(make=make, Z=np.array(d["Z"]), jac=int(name == "dint_var"), n=13)
        if name == "covid":
            from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
            M, params = 10, [3.4, 14, 5, 1, 0.1, 1, -10, 20]
            probe = capi.Context(capi.MODEL_COVID19)
            probe.set_params(params)
            probe.set_step_number(50)
            Xi = np.array([0.93, 0.003, 0.01, 0.057, -0.001, 0.001, 0.0, 0.0])
            time = np.array([30.0 * i / M for i in range(M + 1)])
            X = np.zeros((M + 1, 8))
            X[0] = Xi
            X[M, 3] = 0.6
            for i in range(1, M):
                X[i] = probe.integrate_batch(0.0, time[i], Xi[None, :])[0]
            probe.close()
            mode_x = np.full((M + 1, 4), CONTINUOUS, dtype=np.int32)
            mode_x[0] = FIXED
            mode_x[M] = [FREE, FREE, FREE, FIXED]
            prob = Problem(4, [FIXED] + [CONTINUOUS] * (M - 1) + [FIXED], mode_x, time, X)

            def make(variant):
                ctx = capi.Context(capi.MODEL_COVID19)
                ctx.set_params(params)
                ctx.set_step_number(50)
                return ctx, prob
            return dict(make=make, Z=ec.perturbed(X[:M].ravel(), 2, 1e-3, seed=13), jac=0, n=80)
        assert name in ("lqr1d_fd", "lqr1d_var")
        from oracle.oracle import Problem, FIXED
        Xn = np.zeros((2, 4))
        Xn[1, 0] = 1.0
        prob = Problem(2, [FIXED, FIXED], np.zeros((2, 2), dtype=np.int32), np.array([0.0, 1.0]), Xn)

        def make(variant):
            capi.plugin_load(PLUGIN)
            return capi.Context(1001, nparams=1), prob
        return dict(make=make, Z=ec.perturbed(np.array([0.1, -0.2, -12.0, -6.0]), 3, 1e-2, seed=14), jac=int(name == "lqr1d_var"), n=4)
    return sr.cached(("model", name), build)


def model_context(c, variant="exact"):
    from socp_amd import capi
    ctx, prob = c["make"](variant)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == c["n"]
    return ctx


def device_jacobians(ctx, Z, jac):
    """J[B][n*n] column-major as socp_fd_jacobian_multi_dev (at (z, F(z)), dedup on) / socp_var_jacobian_multi_dev return it."""
    import torch
    B, n = Z.shape
    dZ, dF, dJ = up(Z), up(np.zeros((B, n))), up(np.zeros((B, n * n)))
    torch.cuda.synchronize()
    if jac == 0:
        ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr())
        ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=True)
    else:
        ctx._chk(ctx.L.socp_var_jacobian_multi_dev(ctx.h, B, C.c_void_p(dZ.data_ptr()), C.c_void_p(dJ.data_ptr())))
    ctx.synchronize()
    return dJ.cpu().numpy()


def run_singular_dev(ctx, Z, jac, scale, colnorm=True, max_sweeps=sr.MAX_SWEEPS):
    """The _dev form on guarded buffers: (sigma, vmin, colnorm, sweeps, info) whole, and the counters' advance."""
    import torch
    Z = np.ascontiguousarray(Z)
    B, n = Z.shape
    dZ, dS, dV, dC, dW, dI = up(Z), up(sentinel(B * n)), up(sentinel(B * n)), up(sentinel(B * n)), up(sentinel_i(B)), up(sentinel_i(B))
    wb = ctx.singular_work_bytes(B)
    assert wb >= 8 * (B * n + B * n * n) and wb % 8 == 0
    work = up(sentinel(wb // 8))
    torch.cuda.synchronize()
    t0, l0 = ctx.counters()
    ctx.singular_batch_dev(B, dZ.data_ptr(), 1e-15, jac, scale, max_sweeps, work.data_ptr(), wb, dS.data_ptr(), dV.data_ptr(),
                           dC.data_ptr() if colnorm else None, dW.data_ptr(), dI.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    t1, l1 = ctx.counters()
    assert np.all(work.cpu().numpy().view(np.uint64)[wb // 8:] == np.uint64(SENT)), "guard words behind the workspace were written"
    return (dS.cpu().numpy().view(np.uint64), dV.cpu().numpy().view(np.uint64), dC.cpu().numpy().view(np.uint64), dW.cpu().numpy(),
            dI.cpu().numpy()), (t1 - t0, l1 - l0)


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("name", ["goddard14", "goddard85", "dint_fd", "dint_var", "covid", "lqr1d_fd", "lqr1d_var"])
def test_singular_batch_reference_order_bit_for_bit(name, scale):
    c = model_case(name)
    Z, jac, n = c["Z"], c["jac"], c["n"]
    B = len(Z)
    ctx = model_context(c)
    # the trajectories of the Jacobian alone, for the counters
    t0 = ctx.counters()[0]
    J = device_jacobians(ctx, Z, jac)
    traj_J = ctx.counters()[0] - t0 - (B * ctx.M if jac == 0 else 0)
    ref = sr.cached(("singular", name, scale), lambda: sr.singular_batch(J, scale, sr.MAX_SWEEPS))
    assert np.all(ref["info"] == 0), ref["info"]
    got, (dt, dl) = run_singular_dev(ctx, Z, jac, scale)
    for key, g in zip(("sigma", "vmin", "colnorm"), got[:3]):
        assert np.all(g[B * n:] == np.uint64(SENT)), key + ": guard words"
        bad = np.argwhere(~same_doubles(g[:B * n], ref[key])).ravel()
        assert len(bad) == 0, (name, scale, key, bad[:5].tolist(), g[:B * n].view(np.float64)[bad[:5]], ref[key].ravel()[bad[:5]])
    assert np.all(got[3][B:] == SENT_I) and np.all(got[4][B:] == SENT_I)
    assert np.array_equal(got[3][:B], ref["sweeps"]) and np.array_equal(got[4][:B], ref["info"])
    # counters: B M trajectories of F0 plus the Jacobian's; the residual, the Jacobian (1 launch, variational 3), the column norms,
    # the decomposition
    assert dt == B * ctx.M + traj_J and dl == (4 if jac == 0 else 6), (dt, dl)
    # without colnorm: nothing is written there; unscaled, its launch is not made
    again, (_, dl2) = run_singular_dev(ctx, Z, jac, scale, colnorm=False)
    assert np.all(again[2] == np.uint64(SENT)) and all(np.array_equal(a, b) for a, b in zip(again[:2] + again[3:], got[:2] + got[3:]))
    assert dl2 == dl - (0 if scale else 1)
    # the Python host form
    r = ctx.singular_batch(Z, jac=jac, scale=scale)
    for key, g in zip(("sigma", "vmin", "colnorm"), got[:3]):
        assert np.array_equal(r[key].ravel().view(np.uint64), g[:B * n]), key
    assert np.array_equal(r["sweeps"], got[3][:B]) and np.array_equal(r["info"], got[4][:B])
    cond = r["sigma"][:, 0] / r["sigma"][:, -1]
    print("%s scale %d: n = %d, sweeps %s, sigma_min %s, cond %s" % (name, scale, n, r["sweeps"].tolist(), ["%.3e" % v for v in r["sigma"][:, -1]],
                                                                     ["%.3e" % v for v in cond]))
    ctx.close()


@pytest.mark.parametrize("name", ["goddard14", "goddard85", "dint_fd"])
def test_singular_batch_fast_flavour_info_and_bounds(name):
    c = model_case(name)
    Z, jac, n = c["Z"], c["jac"], c["n"]
    B = len(Z)
    ctx = model_context(c, "fast")
    J = device_jacobians(ctx, Z, jac)                             # the J of the same context
    for scale in (0, 1):
        got, _ = run_singular_dev(ctx, Z, jac, scale)
        assert np.all(got[4][:B] == 0) and np.all(got[0][B * n:] == np.uint64(SENT)) and np.all(got[1][B * n:] == np.uint64(SENT))
        sigma, vmin = got[0][:B * n].view(np.float64).reshape(B, n), got[1][:B * n].view(np.float64).reshape(B, n)
        Js, colnorm = sr.column_scale(J) if scale else (J, np.ones((B, n)))
        assert np.allclose(got[2][:B * n].view(np.float64).reshape(B, n), colnorm, rtol=4 * n * sr.EPS, atol=0)
        for b in range(B):
            q = sr.accuracy_ratios(Js[b], sigma[b], vmin[b])
            print("fast %s scale %d row %d: ratios %.3f %.3f %.3f" % ((name, scale, b) + q))
            assert max(q) <= CB, (name, scale, b, q)
    ctx.close()


def test_singular_batch_blocks_form_equals_row_by_row_and_restores_the_context():
    from socp_amd import capi
    c = ec.case("goddard_blocks")
    rows = [0, 1, 64, 129]
    Z = np.ascontiguousarray(np.asarray(c["Z"])[rows])
    pp, tt, xx = (np.ascontiguousarray(a[rows]) for a in c["blocks"])
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(8)
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == 85
    params_before, tl_before = ctx.get_params().copy(), ctx.timeline(Z[0]).copy()
    F_before = ctx.residual_batch(Z)
    t0, l0 = ctx.counters()
    whole = ctx.singular_batch(Z, scale=1, params=pp, time=tt, xnode=xx)
    t1, l1 = ctx.counters()
    assert np.all(whole["info"] == 0) and l1 - l0 == 4
    shared = ctx.singular_batch(Z, scale=1)
    assert ctx.counters()[0] - t1 == t1 - t0, "the same trajectories with and without blocks"
    assert not np.array_equal(shared["sigma"], whole["sigma"]), "the blocks were in force"
    for k in range(len(rows)):
        one = ctx.singular_batch(Z[k:k + 1], scale=1, params=pp[k:k + 1], time=tt[k:k + 1], xnode=xx[k:k + 1])
        for key in ("sigma", "vmin", "colnorm", "sweeps", "info"):
            assert np.array_equal(one[key][0], whole[key][k]), (k, key)
    # parameters alone: the row-by-row call through the context's own parameters
    only_p = ctx.singular_batch(Z[:2], scale=0, params=pp[:2])
    for k in range(2):
        ctx.set_params(pp[k, :8])
        one = ctx.singular_batch(Z[k:k + 1], scale=0)
        assert np.array_equal(one["sigma"][0], only_p["sigma"][k]) and np.array_equal(one["vmin"][0], only_p["vmin"][k])
    ctx.set_params(params_before)
    # the context's own blocks and parameters are back
    assert np.array_equal(ctx.get_params(), params_before) and np.array_equal(ctx.timeline(Z[0]), tl_before)
    assert np.array_equal(ctx.residual_batch(Z), F_before)
    ctx.close()


def test_singular_batch_refusals_leave_the_context_unchanged():
    from socp_amd import capi
    DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
    c = model_case("dint_fd")
    ctx = model_context(c)
    Z = np.ascontiguousarray(c["Z"])
    B, n = Z.shape
    S, V, Cn, W, I = sentinel(B * n), sentinel(B * n), sentinel(B * n), sentinel_i(B), sentinel_i(B)
    L, h = ctx.L, ctx.h
    zp = Z.ctypes.data_as(DP)
    out = (S.ctypes.data_as(DP), V.ctypes.data_as(DP), Cn.ctypes.data_as(DP), W.ctypes.data_as(IP), I.ctypes.data_as(IP))

    def call(B_=B, Z_=zp, jac=0, scale=0, sweeps_=60, out_=out):
        return L.socp_singular_batch(h, B_, Z_, 1e-15, jac, scale, sweeps_, *out_)
    before = ctx.counters()
    assert call(B_=-1) == capi.ERR_ARG and call(jac=2) == capi.ERR_ARG and call(jac=-1) == capi.ERR_ARG
    assert call(scale=2) == capi.ERR_ARG and call(scale=-1) == capi.ERR_ARG and call(sweeps_=0) == capi.ERR_ARG and call(sweeps_=1001) == capi.ERR_ARG
    assert call(Z_=None) == capi.ERR_ARG
    for k in (0, 1, 3, 4):
        assert call(out_=tuple(None if i == k else o for i, o in enumerate(out))) == capi.ERR_ARG, k
    wb = ctx.singular_work_bytes(B)
    assert wb > 0 and ctx.singular_work_bytes(-1) == 0 and ctx.singular_work_bytes(0) == 0
    fake = C.c_void_p(256)              # never dereferenced: every call below is refused before anything is enqueued
    dev = lambda Z_=fake, work=fake, bytes_=wb, s=fake, v=fake, w=fake, i=fake: L.socp_singular_batch_dev(h, B, Z_, 1e-15, 0, 1, 60, work, bytes_, s, v, None, w, i)  # noqa: E731
    assert dev(Z_=None) == capi.ERR_ARG and dev(work=None) == capi.ERR_ARG and dev(s=None) == capi.ERR_ARG and dev(v=None) == capi.ERR_ARG
    assert dev(w=None) == capi.ERR_ARG and dev(i=None) == capi.ERR_ARG
    assert dev(bytes_=wb - 1) == capi.ERR_ARG and "socp_singular_work_bytes" in L.socp_last_error(h).decode()
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for stride in (3, 4, 6):
        assert L.socp_singular_batch_blocks(h, B, zp, params.ctypes.data_as(DP), stride, None, None, 1e-15, 0, 0, 60, *out) == capi.ERR_ARG, stride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    # B == 0: SOCP_OK without a launch, in all forms
    assert call(B_=0, Z_=None, out_=(None,) * 5) == capi.OK
    assert L.socp_singular_batch_dev(h, 0, None, 1e-15, 0, 0, 60, None, 0, None, None, None, None, None) == capi.OK
    assert L.socp_singular_batch_blocks(h, 0, None, None, 0, None, None, 1e-15, 0, 0, 60, None, None, None, None, None) == capi.OK
    assert ctx.counters() == before, "the refused calls launched and counted nothing"
    for a in (S, V, Cn):
        assert np.all(a.view(np.uint64) == np.uint64(SENT)), "a refused call wrote"
    assert np.all(W == SENT_I) and np.all(I == SENT_I)
    ctx.close()
    # no problem set
    fresh = capi.Context(capi.MODEL_GODDARD)
    assert L.socp_singular_batch(fresh.h, B, zp, 1e-15, 0, 0, 60, *out) == capi.ERR_ARG and "no problem set" in L.socp_last_error(fresh.h).decode()
    assert fresh.singular_work_bytes(1) == 0
    fresh.close()
    # jac = 1 on a model without variational equations
    g = model_case("goddard14")
    gctx = model_context(g)
    gz = np.ascontiguousarray(g["Z"][:1])
    assert L.socp_singular_batch(gctx.h, 1, gz.ctypes.data_as(DP), 1e-15, 1, 0, 60, *out) == capi.ERR_UNSUPPORTED
    assert "variational" in L.socp_last_error(gctx.h).decode() and gctx.counters() == (0, 0)
    gctx.close()
    # n above the LDS bound: the covid19 problem of testCovid19, n = 160
    k = ec.case("covid_m20")
    kctx = capi.Context(capi.MODEL_COVID19)
    kctx.set_params(k["params"])
    kctx.set_step_number(k["N"])
    assert kctx.problem_set(k["prob"].mode_t, k["prob"].mode_x, k["prob"].time, k["prob"].xnode) == 160
    kz = np.ascontiguousarray(k["Z"][:1])
    big = (sentinel(160), sentinel(160), sentinel(160), sentinel_i(1), sentinel_i(1))
    rc = L.socp_singular_batch(kctx.h, 1, kz.ctypes.data_as(DP), 1e-15, 0, 0, 60, big[0].ctypes.data_as(DP), big[1].ctypes.data_as(DP),
                               big[2].ctypes.data_as(DP), big[3].ctypes.data_as(IP), big[4].ctypes.data_as(IP))
    assert rc == capi.ERR_UNSUPPORTED and "160 KiB" in L.socp_last_error(kctx.h).decode() and kctx.counters() == (0, 0)
    assert np.all(big[0].view(np.uint64) == np.uint64(SENT)) and np.all(big[3] == SENT_I)
    kctx.close()
    assert np.all(S.view(np.uint64) == np.uint64(SENT)) and np.all(I == SENT_I)


# ---- 6. the sweep tool ----------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_singular_values_of_its_converged_chains(tmp_path):
    out = str(tmp_path / "sing")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "256", "--rk4-steps", "20", "--sing-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["singular"]
    for key in ("rows", "not_converged", "sigma_min_min", "sigma_min_median", "cond_median", "cond_max"):
        assert key in entry, key
    npz = np.load(entry["file"])
    assert sorted(npz.files) == ["colnorm", "index", "info", "sigma", "sweeps", "vmin"]
    k = entry["rows"]
    assert entry["file"] == out + ".rank0.npz" and k == rec["converged"] > 0 and entry["scale"] == 1 and entry["max_sweeps"] == 60
    assert npz["sigma"].shape == (k, 14) and npz["vmin"].shape == (k, 14) and npz["colnorm"].shape == (k, 14)
    assert npz["info"].shape == (k,) and npz["sweeps"].shape == (k,) and len(set(npz["index"].tolist())) == k and npz["index"].max() < 256
    good = npz["info"] == 0
    assert entry["not_converged"] == int(np.sum(~good)) == 0
    smin = npz["sigma"][good, -1]
    assert entry["sigma_min_min"] == float(smin.min()) > 0 and entry["sigma_min_median"] == float(np.median(smin))
    cond = npz["sigma"][good, 0] / smin
    assert entry["cond_median"] == float(np.median(cond)) and entry["cond_max"] == float(cond.max()) >= 1.0
    assert np.all(np.diff(npz["sigma"], axis=1) <= 0) and np.allclose(np.linalg.norm(npz["vmin"], axis=1), 1.0, rtol=0, atol=1e-13)
    print("sweep --sing-out: %d rows, sigma_min min %.3e median %.3e, cond median %.3e max %.3e" % (
        k, entry["sigma_min_min"], entry["sigma_min_median"], entry["cond_median"], entry["cond_max"]))
    # argument errors, before any device work
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--sing-out", out, "--sing-scale", "3"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "--sing-scale" in bad.stderr
