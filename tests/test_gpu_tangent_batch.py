"""GPU: socp_tangent_batch[_dev] / _blocks and socp_linsolve_batch_dev (capi.Context.tangent_batch, linsolve_batch_dev) against
tests/tangent_reference.py -- steps 1-6 of include/socp_hip.h restated in numpy on the CPU oracle.  Outputs live in sentinel-filled
buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions of test_gpu_events_batch.py); the
workspace is followed by a guard too.
Reference-order flavour: dZ, info and Fp bit-equal to the restatement (NaN compares equal to NaN: the payload of an arithmetic NaN
is the processor's).  Throughput flavour: info equal, the backward error of the solve against the restatement's on the same J and G,
the second-order predictor check of test_tangent_cpu.py on the device's own residual and Jacobian; the deviation of dz from the
reference-order flavour is printed (profiles/tangent_gpu_tests.txt keeps the figures) and not asserted: cond(J) ~ 1e7 amplifies
the flavours' rounding-level difference in J."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import events_cases as ec
import tangent_reference as tr
from tangent_reference import DIR_PARAM, DIR_TIME, DIR_XNODE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0x7FF8DEADBEEF0001                       # a NaN no kernel produces
SENT_I = 0x5EADBEE1
GUARD = 64
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)
MODEL = {"goddard": 1, "dint": 2, "covid": 3}


def sentinel(size):
    return np.full(size + GUARD, np.uint64(SENT), dtype=np.uint64).view(np.float64)


def sentinel_i(size):
    return np.full(size + GUARD, SENT_I, dtype=np.int32)


def ip(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(IP)


# ---- the cases: (case dict, directions, per-row blocks), and their references, computed once ---------------------------------

def case(name):
    def build():
        if name in ("dint", "dint_var"):
            c = dict(tr.dint_case())
            c["dirs"], c["blocks"], c["jac"] = [(DIR_PARAM, 2), (DIR_TIME, 0), (DIR_XNODE, 12)], None, int(name == "dint_var")
        elif name == "goddard_blocks":
            c = dict(ec.case("goddard_blocks"))
            c["dirs"], c["jac"], c["nparams"] = [(DIR_PARAM, 2), (DIR_PARAM, 0)], 0, 8           # KD and C
        else:
            c = dict(ec.case("covid_m20"))
            c["dirs"], c["jac"], c["nparams"] = [(DIR_PARAM, 0), (DIR_XNODE, 3), (DIR_TIME, 20)], 0, 8
        blocks = c["blocks"] or (None, None, None)
        c["ref"] = tr.tangent_reference(c["o"], c["prob"], c["nparams"], c["Z"], c["dirs"], jac=c["jac"], params=blocks[0], time=blocks[1],
                                        xnode=blocks[2])
        return c
    return tr.cached(("gpu", name), build)


def context(c, variant="exact"):
    from socp_amd import capi
    ctx = capi.Context(MODEL[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


def up(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


class DevBlocks:
    """The case's per-row blocks uploaded and in force (socp_problem_set_blocks_dev) inside the with-block."""

    def __init__(self, ctx, blocks):
        self.ctx, self.blocks = ctx, blocks

    def __enter__(self):
        if self.blocks is not None:
            self.keep = [up(a) for a in self.blocks]
            self.ctx._chk(self.ctx.L.socp_problem_set_blocks_dev(self.ctx.h, self.keep[0].data_ptr(), self.blocks[0].shape[1], self.keep[1].data_ptr(),
                                                                 self.keep[2].data_ptr()))
        return self

    def __exit__(self, *exc):
        if self.blocks is not None:
            self.ctx.L.socp_problem_set_blocks_dev(self.ctx.h, None, 0, None, None)


def run_dev(ctx, c, fp=True, Z=None):
    """The _dev form on guarded device buffers: the WHOLE buffers (dZ, info, Fp) back as integer views."""
    import torch
    Z = np.ascontiguousarray(c["Z"] if Z is None else Z)
    B, K, n = len(Z), len(c["dirs"]), ctx.n
    dZ, dD, dI, dF = up(Z), up(sentinel(B * K * n)), up(sentinel_i(B)), up(sentinel(B * K * n))
    wb = ctx.tangent_work_bytes(B, K)
    assert wb > 0 and wb % 8 == 0
    work = up(sentinel(wb // 8))
    with DevBlocks(ctx, c["blocks"]):
        torch.cuda.synchronize()
        ctx.tangent_batch_dev(B, dZ.data_ptr(), c["dirs"], 1e-15, c["jac"], work.data_ptr(), wb, dD.data_ptr(), dI.data_ptr(),
                              dF.data_ptr() if fp else None)
        ctx.synchronize()
        torch.cuda.synchronize()
    assert np.all(work.cpu().numpy().view(np.uint64)[wb // 8:] == np.uint64(SENT)), "guard words behind the workspace were written"
    return dD.cpu().numpy().view(np.uint64), dI.cpu().numpy(), dF.cpu().numpy().view(np.uint64)


def run_host(ctx, c, fp=True, blocks_form=False):
    Z = np.ascontiguousarray(c["Z"])
    B, K, n = len(Z), len(c["dirs"]), ctx.n
    D, I, F = sentinel(B * K * n), sentinel_i(B), sentinel(B * K * n)
    kinds, index = [d[0] for d in c["dirs"]], [d[1] for d in c["dirs"]]
    tail = (K, ip(kinds), ip(index), 1e-15, c["jac"], D.ctypes.data_as(DP), I.ctypes.data_as(IP), F.ctypes.data_as(DP) if fp else None)
    if blocks_form:
        pp, tt, xx = (np.ascontiguousarray(a) for a in c["blocks"])
        ctx._chk(ctx.L.socp_tangent_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), pp.ctypes.data_as(DP), pp.shape[1], tt.ctypes.data_as(DP),
                                                 xx.ctypes.data_as(DP), *tail))
    else:
        ctx._chk(ctx.L.socp_tangent_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    return D.view(np.uint64), I, F.view(np.uint64)


def same_doubles(got, want):
    """Bit equality, a NaN equal to any NaN."""
    g, w = got.view(np.float64), np.ascontiguousarray(want, dtype=np.float64).ravel()
    return (got == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))


def check_whole(got, ref, what, fp=True):
    for name, g, w, fill in (("dZ", got[0], ref["dz"], np.uint64(SENT)), ("info", got[1], ref["info"], SENT_I), ("Fp", got[2], ref["fp"], np.uint64(SENT))):
        if name == "Fp" and not fp:
            assert np.all(g == fill), "%s: Fp was written although its pointer was NULL" % what
            continue
        w = np.ascontiguousarray(w).ravel()
        assert np.all(g[w.size:] == fill), "%s: guard words behind %s were written" % (what, name)
        ok = same_doubles(g[:w.size], w) if w.dtype == np.float64 else g[:w.size] == w
        bad = np.argwhere(~ok).ravel()
        assert len(bad) == 0, (what, name, "%d differ, first flat indices:" % len(bad), bad[:5].tolist(), g[:w.size][bad[:5]], w[bad[:5]])


# ---- 1. reference-order flavour, bit for bit ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dint", "dint_var", "goddard_blocks", "covid"])
def test_reference_order_bit_for_bit(name):
    """dint: B = 3, n = 13, one direction of each kind (four problems per workgroup); dint_var: the variational Jacobian;
    goddard_blocks: B = 130, n = 85, per-row blocks, two wavefronts per matrix in LDS; covid: n = 160, the HBM path."""
    c = case(name)
    ref = c["ref"]
    assert np.all(ref["info"] == 0) and np.all(np.isfinite(ref["dz"])) and np.all(np.max(np.abs(ref["dz"]), axis=2) > 0)
    if name == "goddard_blocks":
        assert ref["swaps"].min() >= 1, "every elimination pivots"
    ctx = context(c)
    assert ctx.n == {"dint": 13, "dint_var": 13, "goddard_blocks": 85, "covid": 160}[name]
    check_whole(run_dev(ctx, c), ref, name + ", _dev form")
    check_whole(run_dev(ctx, c, fp=False), ref, name + ", _dev form, NULL Fp", fp=False)
    ctx.close()


# ---- 2. the elimination on crafted matrices -----------------------------------------------------------------------------------

def crafted(n, K):
    """130 matrices A[b][i][j] and right-hand sides Y[b][K][n]; rows 0 .. 5 are special (see the test), the rest random."""
    def build():
        rng = np.random.default_rng(1000 * n + K)
        A = rng.standard_normal((130, n, n))
        Y = rng.standard_normal((130, K, n))
        A[0] *= 0.01                                            # a swap at every step: the large entries sit one below the diagonal
        for j in range(n):
            A[0, (j + 1) % n, j] = 10.0 * (1.0 + j / n)
        if n > 1:                                               # equal-magnitude candidates: the lowest index wins
            lo, hi = min(2, n - 1), min(5, n - 1)
            A[1, :, 0] *= 0.1
            A[1, lo, 0], A[1, hi, 0] = -3.0, 3.0
        A[2, :, n // 2] = 0.0                                   # exactly singular: no pivot at step n // 2
        A[3, n - 1, n // 2] = np.nan
        Y[4, K - 1, n // 3] = np.inf                            # only the solution is not finite
        A[5, n - 1, n - 1] = np.inf                             # an infinite pivot candidate at the last step
        X, info = tr.eliminate_batch(A, Y)
        swaps = tr.eliminate(A[0], Y[0])[2]
        return A, Y, X, info, swaps
    return tr.cached(("crafted", n, K), build)


@pytest.mark.parametrize("B", [1, 5, 130])
@pytest.mark.parametrize("K", [1, 16])
@pytest.mark.parametrize("n", [1, 13, 64, 65, 127, 160])
def test_linsolve_on_crafted_matrices_bit_for_bit(n, K, B):
    import torch
    from socp_amd import capi
    A, Y, X, info, swaps = crafted(n, K)
    assert swaps == n - 1, "row 0 swaps at every step that has a row below"
    assert info[2] == n // 2 + 1 and np.all(np.isnan(X[2])) and info[1] == 0 and info[0] == 0
    assert n // 2 + 1 <= info[3] <= n + 1 and info[4] == n + 1 and info[5] == n and np.all(info[6:] == 0)
    ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    dA = up(np.concatenate([np.ascontiguousarray(np.transpose(A[:B], (0, 2, 1))).ravel(), sentinel(0)]))     # column-major per problem
    dY = up(np.concatenate([Y[:B].ravel(), sentinel(0)]))
    dI = up(sentinel_i(B))
    torch.cuda.synchronize()
    launches = ctx.counters()[1]
    ctx.linsolve_batch_dev(B, n, K, dA.data_ptr(), dY.data_ptr(), dI.data_ptr())
    ctx.synchronize()
    torch.cuda.synchronize()
    assert ctx.counters()[1] == launches + 1
    gY, gI, gA = dY.cpu().numpy().view(np.uint64), dI.cpu().numpy(), dA.cpu().numpy().view(np.uint64)
    assert np.all(gY[B * K * n:] == np.uint64(SENT)) and np.all(gI[B:] == SENT_I) and np.all(gA[B * n * n:] == np.uint64(SENT)), "guard words"
    T, lda = (4 if n <= 16 else 1), n | 1
    if 8 * T * (lda * (n + K) + 16) <= 64 * 1024:                # the LDS path leaves A as it was; on the HBM path its content is unspecified
        assert np.array_equal(gA[:B * n * n], np.ascontiguousarray(np.transpose(A[:B], (0, 2, 1))).ravel().view(np.uint64)), "A was written on the LDS path"
    else:
        assert n >= 127
    assert np.array_equal(gI[:B], info[:B]), (gI[:B][gI[:B] != info[:B]], info[:B][gI[:B] != info[:B]])
    ok = same_doubles(gY[:B * K * n], X[:B])
    bad = np.argwhere(~ok).ravel()
    assert len(bad) == 0, ("rows", sorted(set((bad // (K * n)).tolist()))[:8], "first", gY[bad[:3]], X[:B].ravel()[bad[:3]])
    ctx.close()


def test_linsolve_with_many_right_hand_sides_and_the_lds_bound():
    """K is not bounded by 16 on this entry point: n = 13 with K = 40 (four problems per workgroup, LDS path) and with K = 600 (HBM
    path); a K whose four pivot rows do not fit the LDS is SOCP_ERR_ARG, before anything is counted or launched."""
    import torch
    from socp_amd import capi
    rng = np.random.default_rng(7)
    ctx = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)
    ctx.set_variant(capi.VARIANT_LANE_EXACT)
    n, B = 13, 5
    for K in (40, 600):
        A, Y = rng.standard_normal((B, n, n)), rng.standard_normal((B, K, n))
        X, info = tr.eliminate_batch(A, Y)
        dA, dY, dI = up(np.ascontiguousarray(np.transpose(A, (0, 2, 1)))), up(np.concatenate([Y.ravel(), sentinel(0)])), up(sentinel_i(B))
        torch.cuda.synchronize()
        ctx.linsolve_batch_dev(B, n, K, dA.data_ptr(), dY.data_ptr(), dI.data_ptr())
        ctx.synchronize()
        gY, gI = dY.cpu().numpy().view(np.uint64), dI.cpu().numpy()
        assert np.all(gY[B * K * n:] == np.uint64(SENT)) and np.all(gI[B:] == SENT_I), "guard words"
        assert np.array_equal(gI[:B], info) and np.all(same_doubles(gY[:B * K * n], X)), K
    before = ctx.counters()
    fake = C.c_void_p(256)              # never dereferenced: the calls are refused
    for K in (2100, 8000, 100000):      # 4 (2 n + K + 16) doubles > 64 KiB
        assert ctx.L.socp_linsolve_batch_dev(ctx.h, B, n, K, fake, fake, fake) == capi.ERR_ARG, K
    assert "64 KiB" in ctx.L.socp_last_error(ctx.h).decode() and ctx.counters() == before
    ctx.close()


# ---- 3. throughput flavour ----------------------------------------------------------------------------------------------------

def device_newton(ctx, z):
    return tr.newton(ctx.residual, lambda x: ctx.fd_jacobian(x, ctx.residual(x), dedup=True), z)


@pytest.mark.parametrize("name", ["dint", "goddard_blocks"])
def test_fast_flavour_info_backward_error_and_predictor(name):
    import torch
    c = case(name)
    ref = c["ref"]
    Z = np.ascontiguousarray(c["Z"])
    B, K, n = len(Z), len(c["dirs"]), Z.shape[1]
    fast = context(c, "fast")
    got = run_dev(fast, c)
    assert np.all(got[0][B * K * n:] == np.uint64(SENT)) and np.all(got[1][B:] == SENT_I) and np.all(got[2][B * K * n:] == np.uint64(SENT)), "guard words"
    assert np.array_equal(got[1][:B], ref["info"]), "info is the reference-order flavour's"
    dz = got[0][:B * K * n].view(np.float64).reshape(B, K, n)
    G = got[2][:B * K * n].view(np.float64).reshape(B, K, n)
    # J of the same context: F0 and the forward-difference Jacobian with the rows' own blocks
    dZ, dF, dJ = up(Z), up(np.zeros((B, n))), up(np.zeros((B, n * n)))
    with DevBlocks(fast, c["blocks"]):
        torch.cuda.synchronize()
        fast.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr())
        fast.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJ.data_ptr(), dedup=True)
        fast.synchronize()
    J = np.transpose(dJ.cpu().numpy().reshape(B, n, n), (0, 2, 1))
    worst, worst_ref = 0.0, 0.0
    for b in range(B):
        be = tr.backward_error(J[b], dz[b], G[b])
        be_ref = tr.backward_error(J[b], tr.eliminate(J[b], -G[b])[0], G[b])
        worst, worst_ref = max(worst, be), max(worst_ref, be_ref)
        assert be <= max(16.0 * be_ref, n * 2.0 ** -53), (b, be, be_ref)
    dev = np.max(np.abs(dz - ref["dz"]), axis=2) / np.max(np.abs(ref["dz"]), axis=2)
    print("fast %s: backward error %.3e (restatement on the same J, G: %.3e; bar max(16 x, n 2^-53 = %.3e)); max |dz_fast - dz_exact| / |dz_exact| = %.3e"
          % (name, worst, worst_ref, n * 2.0 ** -53, float(dev.max())))

    # the second-order predictor check on the device's own residual and Jacobian (shared parameters, the polished golden row)
    from oracle.oracle import Problem
    base = tr.dint_case() if name == "dint" else tr.goddard_case()
    prob = base["prob"]
    z0 = device_newton(fast, base["Z"][0])
    if name == "dint":
        d, theta, fractions = (DIR_XNODE, 12), prob.xnode[1, 0], [0.04, 0.02, 0.01]

        def solve_at(value, start):
            X = prob.xnode.copy()
            X[1, 0] = value
            fast.problem_set(prob.mode_t, prob.mode_x, prob.time, X)
            try:
                return device_newton(fast, start)
            finally:
                fast.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode)
    else:
        d, theta, fractions = (DIR_PARAM, 0), base["params"][0], [0.02, 0.01, 0.005]

        def solve_at(value, start):
            p = np.array(base["params"])
            p[0] = value
            fast.set_params(p)
            try:
                return device_newton(fast, start)
            finally:
                fast.set_params(base["params"])
    t = fast.tangent_batch(z0[None, :], [d])
    assert t["info"][0] == 0
    first, zero = tr.predictor_errors(solve_at, z0, t["dz"][0, 0], theta, fractions)
    tr.check_second_order(first, zero, "fast %s on the device" % name)
    fast.close()


# ---- 4. host forms, restored blocks, counters ---------------------------------------------------------------------------------

def test_host_forms_equal_the_dev_form_and_counters():
    c = case("goddard_blocks")
    ctx = context(c)
    B, K, M = len(c["Z"]), len(c["dirs"]), ctx.M
    want = run_dev(ctx, c)
    got = run_host(ctx, c, blocks_form=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), "_blocks form"
    # the context's own blocks are back: the plain host form is the shared-parameter call, and equals the _dev form without blocks
    plain = dict(c, blocks=None)
    shared = run_host(ctx, plain)
    assert not np.array_equal(shared[0], want[0])
    assert all(np.array_equal(a, b) for a, b in zip(shared, run_dev(ctx, plain))), "host form"
    # NULL Fp through the host form
    nofp = run_host(ctx, plain, fp=False)
    assert np.array_equal(nofp[0], shared[0]) and np.array_equal(nofp[1], shared[1]) and np.all(nofp[2] == np.uint64(SENT))
    # the Python form
    t = ctx.tangent_batch(c["Z"], c["dirs"], params=c["blocks"][0], time=c["blocks"][1], xnode=c["blocks"][2], fp=True)
    n = ctx.n
    assert np.array_equal(t["dz"].ravel().view(np.uint64), want[0][:B * K * n]) and np.array_equal(t["info"], want[1][:B])
    assert np.array_equal(t["fp"].ravel().view(np.uint64), want[2][:B * K * n])
    # counters: B (K + 1) M trajectories of the residual launch and the dedup list's of the Jacobian; five launches
    z, F = np.ascontiguousarray(c["Z"][0]), ctx.residual(c["Z"][0])
    t0, _ = ctx.counters()
    ctx.fd_jacobian(z, F, dedup=True)
    T_dedup = ctx.counters()[0] - t0
    t0, l0 = ctx.counters()
    run_dev(ctx, plain)
    t1, l1 = ctx.counters()
    assert t1 - t0 == B * (K + 1) * M + B * T_dedup and l1 - l0 == 5
    ctx.close()
    # variational: B M trajectories and three launches for the Jacobian
    v = case("dint_var")
    vctx = context(v)
    t0, l0 = vctx.counters()
    run_dev(vctx, v)
    t1, l1 = vctx.counters()
    Bv, Kv = len(v["Z"]), len(v["dirs"])
    assert t1 - t0 == Bv * (Kv + 1) * vctx.M + Bv * vctx.M and l1 - l0 == 7
    vctx.close()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_unchanged():
    from socp_amd import capi
    c = case("dint")
    ctx = context(c)
    Z = np.ascontiguousarray(c["Z"])
    B, n, M, S, d = len(Z), ctx.n, ctx.M, ctx.s, ctx.dim
    D, I, F = sentinel(B * 16 * n), sentinel_i(B), sentinel(B * 16 * n)
    L, h = ctx.L, ctx.h
    zp, out = Z.ctypes.data_as(DP), (D.ctypes.data_as(DP), I.ctypes.data_as(IP), F.ctypes.data_as(DP))

    def call(B_=B, Z_=zp, kinds=(0,), index=(0,), K=None, jac=0, out_=out):
        K = (len(kinds) if kinds is not None else 1) if K is None else K
        return L.socp_tangent_batch(h, B_, Z_, K, ip(kinds) if kinds is not None else None, ip(index) if index is not None else None, 1e-15, jac, *out_)
    before = ctx.counters()
    tl = ctx.timeline(Z[0]).copy()
    assert call(B_=-1) == capi.ERR_ARG
    assert call(kinds=(), index=(), K=0) == capi.ERR_ARG and call(kinds=(0,) * 17, index=(0,) * 17) == capi.ERR_ARG
    assert call(kinds=(3,)) == capi.ERR_ARG and call(kinds=(-1,)) == capi.ERR_ARG
    for kind, index in ((0, 5), (0, -1), (1, M + 1), (1, -1), (2, (M + 1) * S), (2, d), (2, S + d), (2, -1)):
        assert call(kinds=(kind,), index=(index,)) == capi.ERR_ARG, (kind, index)
    for kind, index in ((0, 4), (1, M), (2, d - 1), (2, S + d - 1)):
        assert call(kinds=(kind,), index=(index,)) == capi.OK, (kind, index)
    after_ok = ctx.counters()
    assert call(Z_=None) == capi.ERR_ARG and call(kinds=None) == capi.ERR_ARG and call(index=None) == capi.ERR_ARG
    assert call(out_=(None, out[1], out[2])) == capi.ERR_ARG and call(out_=(out[0], None, out[2])) == capi.ERR_ARG
    assert call(jac=2) == capi.ERR_ARG
    # _dev: NULL pointers, a workspace one byte short
    wb = ctx.tangent_work_bytes(B, 1)
    assert wb > 0 and ctx.tangent_work_bytes(B, 0) == 0 and ctx.tangent_work_bytes(B, 17) == 0 and ctx.tangent_work_bytes(-1, 1) == 0
    fake = C.c_void_p(256)              # never dereferenced: every call below is refused before anything is enqueued
    dev = lambda Z_=fake, work=fake, bytes_=wb, dZ=fake, info=fake: L.socp_tangent_batch_dev(h, B, Z_, 1, ip([0]), ip([0]), 1e-15, 0, work, bytes_, dZ, info, None)  # noqa: E731
    assert dev(Z_=None) == capi.ERR_ARG and dev(work=None) == capi.ERR_ARG and dev(dZ=None) == capi.ERR_ARG and dev(info=None) == capi.ERR_ARG
    assert dev(bytes_=wb - 1) == capi.ERR_ARG and "socp_tangent_work_bytes" in L.socp_last_error(h).decode()
    # _blocks: the stride
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for stride in (3, 4, 6):
        assert L.socp_tangent_batch_blocks(h, B, zp, params.ctypes.data_as(DP), stride, None, None, 1, ip([0]), ip([0]), 1e-15, 0, *out) == capi.ERR_ARG, stride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    # B == 0: SOCP_OK without a launch, in all forms
    assert call(B_=0, Z_=None, out_=(None, None, None)) == capi.OK
    assert L.socp_tangent_batch_dev(h, 0, None, 1, ip([0]), ip([0]), 1e-15, 0, None, 0, None, None, None) == capi.OK
    assert L.socp_tangent_batch_blocks(h, 0, None, None, 0, None, None, 1, ip([0]), ip([0]), 1e-15, 0, None, None, None) == capi.OK
    # the linear solve on its own
    for args in ((-1, 3, 1), (1, 0, 1), (1, 3, 0), (1, 5000, 1)):
        assert L.socp_linsolve_batch_dev(h, args[0], args[1], args[2], fake, fake, fake) == capi.ERR_ARG, args
    assert L.socp_linsolve_batch_dev(h, 1, 3, 1, None, fake, fake) == capi.ERR_ARG and L.socp_linsolve_batch_dev(h, 1, 3, 1, fake, None, fake) == capi.ERR_ARG
    assert L.socp_linsolve_batch_dev(h, 1, 3, 1, fake, fake, None) == capi.ERR_ARG and L.socp_linsolve_batch_dev(h, 0, 3, 1, None, None, None) == capi.OK
    assert ctx.counters() == after_ok, "the refused calls launched and counted nothing"
    assert after_ok != before and np.array_equal(ctx.timeline(Z[0]), tl)
    # no problem set; a model without variational equations
    fresh = capi.Context(capi.MODEL_GODDARD)
    assert L.socp_tangent_batch(fresh.h, B, zp, 1, ip([0]), ip([0]), 1e-15, 0, *out) == capi.ERR_ARG and "no problem set" in L.socp_last_error(fresh.h).decode()
    assert fresh.tangent_work_bytes(1, 1) == 0
    fresh.close()
    g = tr.goddard_case()
    gctx = context(g)
    gz = np.ascontiguousarray(g["Z"])
    gD, gI = sentinel(85), sentinel_i(1)
    assert L.socp_tangent_batch(gctx.h, 1, gz.ctypes.data_as(DP), 1, ip([0]), ip([0]), 1e-15, 1, gD.ctypes.data_as(DP), gI.ctypes.data_as(IP), None) == capi.ERR_UNSUPPORTED
    assert "variational" in L.socp_last_error(gctx.h).decode() and np.all(gD.view(np.uint64) == np.uint64(SENT)) and gctx.counters() == (0, 0)
    gctx.close()
    # a valid call afterwards gives the reference's bits
    check_whole(run_host(ctx, c), c["ref"], "after the refused calls")
    ctx.close()


# ---- 6. the sweep tool ----------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_tangents_of_its_converged_chains(tmp_path):
    from socp_amd import capi, sweep
    out = str(tmp_path / "tan")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "100", "--tangent-out", out, "--tangent-param", "C"],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["tangent_rank0"]
    assert sorted(entry) == sorted(["parameter", "chains", "info_nonzero", "median_norm_dz", "wall_s", "file"])
    npz = np.load(entry["file"])
    assert sorted(npz.files) == ["dz", "index", "info", "theta", "z"]
    k = entry["chains"]
    assert entry["file"] == out + ".rank0.npz" and entry["parameter"] == "C" and k == rec["converged"] > 0
    assert npz["dz"].shape == (k, 14) and npz["z"].shape == (k, 14) and npz["info"].shape == (k,) and npz["index"].shape == (k,)
    assert np.all(npz["theta"] == sweep.GODDARD_PARAMS[0]) and len(set(npz["index"].tolist())) == k and npz["index"].max() < 64
    solved = npz["info"] == 0
    assert entry["info_nonzero"] == int(np.sum(~solved)) == 0
    assert entry["median_norm_dz"] == float(np.median(np.linalg.norm(npz["dz"][solved], axis=1))) > 0
    ctx = capi.Context(capi.MODEL_GODDARD)
    ctx.set_params(sweep.GODDARD_PARAMS)
    ctx.set_step_number(100)
    ctx.set_variant(capi.VARIANT_LANE_FAST)
    sweep.goddard_single_shooting_problem(ctx)
    direct = ctx.tangent_batch(npz["z"], [(capi.DIR_PARAM, capi.GODDARD_PARAM_NAMES.index("C"))])
    assert np.array_equal(direct["info"], npz["info"])
    assert np.array_equal(direct["dz"][:, 0, :].ravel().view(np.uint64), np.ascontiguousarray(npz["dz"]).ravel().view(np.uint64))
    ctx.close()
    # argument errors, before any device work
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--tangent-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--tangent-out" in bad.stderr
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--tangent-out", out, "--tangent-param", "nosuch"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--tangent-param" in bad.stderr
