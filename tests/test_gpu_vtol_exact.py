"""GPU: vtolUAV in the exact-derivative stack -- socp_fields_batch, socp_exact_jacobian_batch and socp_newton_batch with jac = 2 on
a SOCP_MODEL_VTOLUAV context (custom final rows through final_row_t, the switching_state rows of a FREE interior component through
switching_state_t) against tests/vtol_exact_reference.py and the fixture tests/golden/vtol_exact_pin.npz.  Stages path_1 (n = 13),
path_2 (n = 26) and, for the structure, path_8 (n = 104) of tests/golden/vtol_flow.npz; ca = alphaV = 0.05, N = 10 steps.
Outputs live in sentinel-filled buffers followed by 64 guard words and are compared WHOLE on integer views (the conventions of
test_gpu_exact_jacobian.py and test_gpu_fields_batch.py); NaNs other than the sentinel are compared as NaN.
(1) EMPTY map -- no tanh is evaluated: every output bit is the restatement's, host, _dev and _blocks forms, both flavours;
(2) shipped map -- tanh is the device library's: F is socp_residual_batch's bits, the continuity blocks are Phi as numbers, the
matrix is within 8 x dev_ref of the fixture's 240-bit matrix (the project's margin for tanh-bearing segments), a forward
difference agrees to its own accuracy, a throughput context returns the same bits, the zero pattern at n = 104;
(3) Newton with jac = 2 from the fixture's starts; (4) what stays refused.
A reference is computed once and shared read-only.  The figures are written to profiles/vtol_exact_gpu_tests.txt.
The entries are switched per context (socp_ctx_set_exact_hooks): a context that has not asked answers as before the model had them.
Without the feature every test fails at the missing symbol."""
import os

import numpy as np
import pytest

import fields_reference as fr
import vtol_exact_reference as vx
import test_gpu_fields_batch as tf
from test_gpu_jacobi_batch import SENT, DP, sentinel, sentinel_i, views, canon
from test_gpu_exact_jacobian import check_whole, matrices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PROFILE = os.path.join(ROOT, "profiles", "vtol_exact_gpu_tests.txt")
PIN = np.load(os.path.join(GOLD, "vtol_exact_pin.npz"))
FLOW = np.load(os.path.join(GOLD, "vtol_flow.npz"))
SHIPPED, EMPTY = PIN["table_shipped"], np.zeros((0, 7))
N = int(PIN["N"])
D, S = vx.D, vx.S
STRIDE, SKIP, CAP = 3, 0, 4                       # the fields: every third step and the last one: 4 samples of 10 steps
_FIG, _REF = {}, {}


def record(key, line):
    print("[vtol_exact_gpu %s] %s" % (key, line))
    _FIG[key] = line
    try:
        with open(PROFILE, "w") as f:
            f.write("tests/test_gpu_vtol_exact.py on an MI355X: vtolUAV stages of tests/golden/vtol_flow.npz, ca = alphaV = 0.05, N = 10 RK4 steps per\n"
                    "segment (pytest -s prints the same lines)\n\n")
            for k in sorted(_FIG):
                f.write("[%s] %s\n" % (k, _FIG[k]))
    except OSError:
        pass


def setting(name):
    if name in vx.STAGES:
        return vx.stage(FLOW, name, ca=vx.CA, alphaV=vx.ALPHAV)
    return vx.stage(FLOW, name)


def context(name, table, variant="exact", P=None):
    from socp_amd import capi
    Pn, prob, _ = setting(name)
    ctx = capi.Context(capi.MODEL_VTOLUAV)
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_exact_hooks(True)                      # the entries are off in a new context (socp_ctx_set_exact_hooks)
    ctx.set_map(table)
    ctx.set_params(Pn if P is None else P)
    ctx.set_step_number(N)
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


def rows_of(name, B):
    """B unknown vectors of a stage: the stored solution, rows moved by up to 1 %, then (B >= 4) a row with a NaN start costate
    and (B >= 5) a row at rest -- rows 9-11 of its right-hand side are NaN, as upstream."""
    _, prob, z = setting(name)
    Z = np.tile(z, (B, 1)) * (1.0 + 0.01 * np.random.default_rng(31).uniform(-1.0, 1.0, size=(B, len(z))))
    Z[0] = z
    if B >= 4:
        Z[3, 9] = np.nan
    if B >= 5:
        Z[4, 3:6] = 0.0
    Z.setflags(write=False)
    return Z


def blocks_of(name, B):
    """Per-row blocks: ca, invSigmaXwp and alphaV differ from row to row, the node states by up to 1 %, the fixed time t0 by a shift."""
    P, prob, _ = setting(name)
    rng = np.random.default_rng(32)
    pp = np.tile(np.concatenate([P, [0.0, 0.0]]), (B, 1))
    pp[:, vx.I_CA] = np.linspace(0.03, 0.07, B)
    pp[:, vx.I_INVSIGMA] = np.linspace(1.0 / 80, 1.0 / 40, B)
    pp[:, vx.I_ALPHAV] = np.linspace(0.02, 0.06, B)
    tt = np.tile(np.asarray(prob.time, dtype=np.float64), (B, 1))
    tt[:, 0] = np.linspace(0.0, 0.2, B)
    xx = np.tile(np.asarray(prob.xnode, dtype=np.float64).ravel(), (B, 1)) * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, size=(B, prob.xnode.size)))
    return pp, tt, xx.reshape(B, -1)


def segment_times(prob, z):
    lay = vx.Layout(prob)
    jt = lambda j: z[lay.kind[j]] if lay.kind[j] >= 0 else prob.time[j]          # noqa: E731
    assert all(k != -2 for k in lay.kind), "every node of these stages is a junction"
    return [(jt(i), jt(i + 1)) for i in range(lay.M)]


def jacobian_reference(name, table_tag, B, blocks=False):
    key = ("jac", name, table_tag, B, blocks)
    if key not in _REF:
        P, prob, _ = setting(name)
        _REF[key] = vx.exact_jacobian_batch(P, SHIPPED if table_tag == "shipped" else EMPTY, prob, rows_of(name, B), N,
                                            blocks=blocks_of(name, B) if blocks else None)
    return _REF[key]


def fields_reference(name, B, blocks=False):
    """slabs[b][i] with all s columns, EMPTY map."""
    from oracle.oracle import Problem
    key = ("fields", name, B, blocks)
    if key not in _REF:
        P, prob, _ = setting(name)
        pp, tt, xx = blocks_of(name, B) if blocks else (None, None, None)
        slabs = []
        for b, z in enumerate(rows_of(name, B)):
            Pb = P if pp is None else pp[b][:len(P)]
            pb = prob if tt is None else Problem(prob.dim, prob.mode_t, prob.mode_x, tt[b], xx[b])
            slabs.append([vx.fields_segment(Pb, EMPTY, t1, t2, z[S * i:S * (i + 1)], N, cols=fr.ALL, stride=STRIDE, skip=SKIP)
                          for i, (t1, t2) in enumerate(segment_times(pb, z))])
        _REF[key] = slabs
    return _REF[key]


def jac_host(ctx, Z, f=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B, n = len(Z), ctx.n
    out = (sentinel(B * n * n), sentinel(B * n))
    tail = (out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP) if f else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_exact_jacobian_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) for a in blocks)
        ctx._chk(ctx.L.socp_exact_jacobian_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), pp.ctypes.data_as(DP), pp.shape[1], tt.ctypes.data_as(DP),
                                                        xx.ctypes.data_as(DP), *tail))
    return views(out)


def jac_dev(ctx, Z, f=True):
    import torch
    B, n = len(Z), ctx.n
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (sentinel(B * n * n), sentinel(B * n))]
    torch.cuda.synchronize()
    ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr() if f else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return views(tuple(t.cpu().numpy() for t in dev))


def fields_expected(name, slabs, cols):
    _, prob, _ = setting(name)
    return tf.expected(dict(prob=prob), slabs, cols, skip=SKIP, cap=CAP)


# ---- 1. EMPTY map: every bit is the restatement's ---------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 4, 5])
def test_empty_map_path_1_equals_the_restatement(B):
    """M = 1: all-FREE custom final rows and the free final time's H row.  Four groups of 13 lanes fill a wavefront: B = 4 is one
    full wave, B = 5 a second one with three idle groups.  Row 3 starts from a NaN, row 4 at rest."""
    Z = rows_of("path_1", B)
    want = jacobian_reference("path_1", "empty", 5)
    want = (want[0][:B], want[1][:B])
    slabs = fields_reference("path_1", 5)[:B]
    for variant in ("exact", "fast"):
        ctx = context("path_1", EMPTY, variant)
        assert ctx.has_exact_jacobian() and ctx.has_fields()
        t0, l0 = ctx.counters()
        check_whole(jac_host(ctx, Z), want, "path_1 B = %d, %s, host form" % (B, variant))
        check_whole(jac_dev(ctx, Z), want, "path_1 B = %d, %s, _dev form" % (B, variant))
        t1, l1 = ctx.counters()
        assert t1 - t0 == 2 * B * (S + 1) and l1 - l0 == 2, "B M (S + 1) trajectories and one launch per call"
        check_whole(jac_dev(ctx, Z, f=False), (want[0], None), "path_1 B = %d, %s, NULL F" % (B, variant))
        for cols in (fr.COSTATE, fr.ALL):
            exp = fields_expected("path_1", slabs, cols)
            tf.check_whole(tf.run_host(ctx, Z, cols, STRIDE, SKIP, CAP), exp, "path_1 B = %d, %s, fields cols %d, host form" % (B, variant, cols))
            tf.check_whole(tf.run_dev(ctx, Z, cols, STRIDE, SKIP, CAP), exp, "path_1 B = %d, %s, fields cols %d, _dev form" % (B, variant, cols))
        ctx.close()
    if B == 5:
        J = want[0].reshape(5, 13, 13)
        assert np.isnan(J[3]).any() and np.isnan(J[4]).any() and np.isfinite(J[:3]).all(), "the NaN row, the row at rest, and only they"
        record("1 path_1", "EMPTY map, B = 1, 4, 5, both flavours: Fjac, F and the six outputs of socp_fields_batch (cols 0 and 1, stride 3) "
               "bit-equal to the restatement, host and _dev forms, NULL F; rows 3 (NaN start) and 4 (at rest) NaN as the restatement")


@pytest.mark.parametrize("B", [2, 3])
def test_empty_map_path_2_equals_the_restatement_with_per_row_blocks(B):
    """M = 2: the interior node's positions FREE (hook rows), its velocities CONTINUOUS, both times FREE."""
    Z = rows_of("path_2", B)
    want = jacobian_reference("path_2", "empty", B)
    ctx = context("path_2", EMPTY)
    check_whole(jac_host(ctx, Z), want, "path_2 B = %d, host form" % B)
    check_whole(jac_dev(ctx, Z), want, "path_2 B = %d, _dev form" % B)
    check_whole(jac_dev(ctx, Z, f=False), (want[0], None), "path_2 B = %d, NULL F" % B)
    slabs = fields_reference("path_2", B)
    for cols in (fr.COSTATE, fr.ALL):
        tf.check_whole(tf.run_dev(ctx, Z, cols, STRIDE, SKIP, CAP), fields_expected("path_2", slabs, cols), "path_2 B = %d, fields cols %d" % (B, cols))
    # per-row blocks
    blocks = blocks_of("path_2", B)
    wantb = jacobian_reference("path_2", "empty", B, blocks=True)
    assert not np.array_equal(wantb[0], want[0])
    check_whole(jac_host(ctx, Z, blocks=blocks), wantb, "path_2 B = %d, _blocks form" % B)
    slabsb = fields_reference("path_2", B, blocks=True)
    for cols in (fr.COSTATE, fr.ALL):
        tf.check_whole(tf.run_host(ctx, Z, cols, STRIDE, SKIP, CAP, blocks=blocks), fields_expected("path_2", slabsb, cols),
                       "path_2 B = %d, fields cols %d, _blocks form" % (B, cols))
    check_whole(jac_host(ctx, Z), want, "path_2 B = %d, the shared blocks again" % B)
    ctx.close()
    record("1 path_2 B=%d" % B, "EMPTY map: Fjac, F and the six outputs of socp_fields_batch bit-equal to the restatement, host, _dev and _blocks forms")


# ---- 2. the shipped map ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", vx.STAGES)
def test_shipped_map_against_the_240_bit_matrix(name):
    P, prob, z = setting(name)
    n, M = len(z), prob.M
    Z = z[None, :]
    ctx = context(name, SHIPPED)
    got = jac_dev(ctx, Z)
    assert np.all(got[0][n * n:] == np.uint64(SENT)) and np.all(got[1][n:] == np.uint64(SENT)), "guard words"
    J = matrices(got[0], 1, n)[0]
    F = got[1][:n].view(np.float64)
    # F: socp_residual_batch of this reference-order context, bit for bit
    Fr = ctx.residual_batch(np.ascontiguousarray(Z))[0]
    assert np.array_equal(canon(F.view(np.uint64).copy()), canon(Fr.view(np.uint64).copy())), "F against socp_residual_batch"
    # the continuity blocks against Phi of socp_fields_batch, as numbers
    phi = ctx.fields_batch(Z, cols=fr.ALL, stride=N, cap=4, phi=True)["phi"].cpu().numpy()[0]
    assert np.isfinite(phi).all()
    inv_sigma = P[vx.I_INVSIGMA]
    for i in range(M - 1):
        blk = J[S * (i + 1):S * (i + 2), S * i:S * (i + 1)]
        for j in range(D):
            mode = prob.mode_x[i + 1][j]
            assert mode != vx.FIXED
            assert np.array_equal(blk[j], phi[i][j]), (name, i, j, "state row")
            want = phi[i][j + D] - inv_sigma * phi[i][j] if mode == vx.FREE else phi[i][j + D]
            assert np.array_equal(blk[j + D], want), (name, i, j, "costate row")
    # the matrix against the fixture's 240-bit one: 8 x the restatement's own deviation (README, the vtolUAV pinning paragraph)
    J240, dev_ref = PIN[name + "_shipped_J240"], float(PIN[name + "_shipped_dev_ref"])
    scale = np.abs(J240).max()
    dev = np.abs(J - J240).max() / scale
    record("2 %s 240-bit" % name, "shipped map, n = %d: max |J - J240| / max|J| = %.3e; dev_ref = %.3e; ratio %.3f of the 8 x allowance; "
           "F bit-equal to socp_residual_batch; continuity blocks equal Phi" % (n, dev, dev_ref, dev / (8 * dev_ref)))
    assert dev <= 8 * dev_ref
    # a throughput-flavour context returns the reference-order context's bits
    cf = context(name, SHIPPED, "fast")
    gf = jac_dev(cf, Z)
    assert np.array_equal(canon(gf[0]), canon(got[0])) and np.array_equal(canon(gf[1]), canon(got[1])), "the throughput flavour's bits"
    cf.close()
    if name == "path_2":
        Jfd = ctx.fd_jacobian(z, Fr, epsfcn=1e-15)
        dfd = np.abs(Jfd - J).max() / scale
        col = np.abs(Jfd - J).max(axis=0) / scale
        record("2 path_2 forward difference", "max over the matrix of |J_fd - J| / max|J| = %.3e (worst column %d; median column %.3e); guard 1e-4"
               % (dfd, int(col.argmax()), float(np.median(col))))
        assert dfd < 1e-4
    ctx.close()


def test_structure_at_n_104():
    """path_8: seven interior nodes with FREE positions.  The zero pattern is the restatement's; the two rows of every hook
    component hold, in the next segment's columns, exactly one -1 each and nothing else."""
    P, prob, z = setting("path_8")
    n, M = len(z), prob.M
    assert n == 104 and M == 8
    ctx = context("path_8", SHIPPED)
    got = jac_dev(ctx, z[None, :])
    J = matrices(got[0], 1, n)[0]
    Jr, _ = vx.exact_jacobian_row(P, SHIPPED, prob, z, N)
    assert np.isfinite(J).all() and np.array_equal(J != 0, Jr != 0), "the zero pattern"
    hooks = 0
    for k in range(1, M):
        for j in range(D):
            if prob.mode_x[k][j] != vx.FREE:
                continue
            hooks += 1
            for row, col in ((S * k + j, S * k + j), (S * k + D + j, S * k + D + j)):
                own = J[row, S * k:S * (k + 1)]
                assert own[col - S * k] == -1.0 and np.count_nonzero(own) == 1, (k, j, row)
    assert hooks == 21
    rel = np.abs(J - Jr).max() / np.abs(Jr).max()
    record("2 path_8 structure", "n = 104: zero pattern equal to the restatement's (%d nonzeros of %d), %d hook components with exactly two -1 "
           "entries in the next segment's columns; max |J - restatement| / max|J| = %.3e" % (int((J != 0).sum()), n * n, hooks, rel))
    ctx.close()


# ---- 3. Newton ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", vx.STAGES)
def test_newton_with_the_exact_jacobian(name):
    from socp_amd import capi
    starts, zref = PIN[name + "_newton_starts"], PIN[name + "_newton_z"]
    ctx = context(name, SHIPPED)
    res = ctx.newton_batch(starts, jac=2)
    err = np.max(np.abs(res["z"] - zref) / np.maximum(1.0, np.abs(zref)))
    record("3 %s" % name, "jac = 2 from the fixture's %d starts (factor %.0e): status %s, iterations %s, max rnorm %.3e, "
           "max |z - z_restatement| / max(1, |z|) = %.3e (bar 1e-8)" % (len(starts), float(PIN["newton_factor"]), sorted(set(res["status"].tolist())),
                                                                       res["iters"].tolist(), res["rnorm"].max(), err))
    assert np.all(res["status"] == capi.NEWTON_CONVERGED)
    assert np.all(np.abs(res["z"] - zref) <= 1e-8 * np.maximum(1.0, np.abs(zref)))
    ctx.close()


# ---- 4. what stays refused ---------------------------------------------------------------------------------------------------------

def test_refusals_unchanged():
    from socp_amd import capi
    _, prob, z = setting("path_2")
    Z = z[None, :]
    for variant in ("exact", "fast"):
        ctx = context("path_2", SHIPPED, variant)
        assert ctx.has_exact_jacobian() and ctx.has_fields()
        assert ctx.L.socp_ctx_has_exact_jacobian(ctx.h) == 1 and ctx.L.socp_ctx_has_fields(ctx.h) == 1
        assert not (ctx.has_gain() or ctx.has_gain_free() or ctx.has_guide() or ctx.has_sensitivity() or ctx.has_jacobi())
        assert not (ctx.has_hamiltonian_gradient() or ctx.has_hamiltonian_jacobian()) and ctx.event_channels() == 0
        calls = {"gain": lambda: ctx.gain_batch(Z), "gain_free": lambda: ctx.gain_free_batch(Z),
                 "guide": lambda: ctx.guide_batch(Z, np.zeros((1, 1, D))),
                 "sensitivity": lambda: ctx.sensitivity_batch(Z, [(capi.DIR_PARAM, 0)]), "jacobi": lambda: ctx.jacobi_batch(Z),
                 "events": lambda: ctx.events_batch(Z, 0, np.zeros((1, 1))),
                 "hamiltonian_gradient": lambda: ctx.hamiltonian_gradient_batch(0.0, Z[:, :S]),
                 "hamiltonian_jacobian": lambda: ctx.hamiltonian_jacobian_batch(0.0, Z[:, :S])}
        c0 = ctx.counters()
        for label, call in calls.items():
            with pytest.raises(capi.SocpError) as err:
                call()
            assert err.value.code == capi.ERR_UNSUPPORTED, (label, str(err.value))
        # the adaptive integrator
        ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
        out = (sentinel(prob.n * prob.n), sentinel(prob.n))
        assert ctx.L.socp_exact_jacobian_batch(ctx.h, 1, Z.ctypes.data_as(DP), out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP)) == capi.ERR_UNSUPPORTED
        assert "DOPRI5" in ctx.L.socp_last_error(ctx.h).decode()
        assert all(np.all(a.view(np.uint64) == np.uint64(SENT)) for a in out), "nothing was written"
        fo = tf.buffers(1, prob.M, CAP, D, fr.ALL)
        assert tf.raw(ctx, 1, np.ascontiguousarray(Z), fr.ALL, STRIDE, SKIP, CAP, fo) == capi.ERR_UNSUPPORTED
        assert "DOPRI5" in ctx.L.socp_last_error(ctx.h).decode()
        with pytest.raises(capi.SocpError) as err:
            ctx.newton_batch(Z, jac=2)
        assert err.value.code == capi.ERR_UNSUPPORTED
        assert ctx.counters() == c0, "nothing was launched or counted"
        ctx.set_integrator(capi.INT_RK4)
        # switched off again, and in a context that never asked: the answers of a model without the two entries
        fresh = context("path_2", SHIPPED, variant)
        fresh.set_exact_hooks(False)
        for cx in (fresh, ctx):
            cx.set_exact_hooks(False)
            assert not cx.has_exact_jacobian() and not cx.has_fields()
            assert cx.L.socp_ctx_has_exact_jacobian(cx.h) == 0 and cx.L.socp_ctx_has_fields(cx.h) == 0
            out = (sentinel(prob.n * prob.n), sentinel(prob.n))
            assert cx.L.socp_exact_jacobian_batch(cx.h, 1, Z.ctypes.data_as(DP), out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP)) == capi.ERR_UNSUPPORTED
            assert "no exact_jacobian entry" in cx.L.socp_last_error(cx.h).decode()
            assert all(np.all(a.view(np.uint64) == np.uint64(SENT)) for a in out), "nothing was written"
            fo = tf.buffers(1, prob.M, CAP, D, fr.ALL)
            assert tf.raw(cx, 1, np.ascontiguousarray(Z), fr.ALL, STRIDE, SKIP, CAP, fo) == capi.ERR_UNSUPPORTED
            assert "no fields entry" in cx.L.socp_last_error(cx.h).decode()
            with pytest.raises(capi.SocpError) as err:
                cx.newton_batch(Z, jac=2)
            assert err.value.code == capi.ERR_UNSUPPORTED
        assert ctx.counters() == c0
        fresh.close()
        ctx.close()
    other = capi.Context(capi.MODEL_DOUBLE_INTEGRATOR)
    with pytest.raises(capi.SocpError) as err:
        other.set_exact_hooks(True)
    assert err.value.code == capi.ERR_UNSUPPORTED and other.has_fields() and other.has_exact_jacobian()
    other.close()
    record("4 refusals", "both flavours: has_exact_jacobian = has_fields = 1 after socp_ctx_set_exact_hooks(ctx, 1) and 0 with the refusals of a model without "
           "the entries before it or after (ctx, 0); gain, gain_free, guide, sensitivity, jacobi, events and the two "
           "Hamiltonian point calls SOCP_ERR_UNSUPPORTED; the adaptive integrator refused by fields, exact Jacobian and Newton (jac = 2)")
