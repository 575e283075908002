"""GPU: the batched exact shooting Jacobian (socp_exact_jacobian_batch[_dev] / _blocks, capi.Context.exact_jacobian_batch) against
tests/exact_jacobian_reference.py -- the definition restated in Python on dual numbers.  Outputs live in sentinel-filled buffers
followed by 64 guard words and are compared WHOLE on integer views (the conventions of test_gpu_fields_batch.py), so a store past a
matrix or through a NULL F shows, and so does the sign of a zero.  Every output is bit-equal to the restatement, in both flavours
(the kernels are one object without contraction); the one exception is the payload of a NaN that arithmetic produced from a NaN
input, so NaNs other than the sentinel are compared as NaN.  N = 10 steps.  A reference is computed once and shared read-only.
The figures the tests print are kept in profiles/exact_jacobian_gpu_tests.txt.  Without the feature every test fails at the missing
symbol."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_jacobian_reference as ej
import fields_reference as fr
import jacobi_cases as jc
from test_gpu_jacobi_batch import SENT, GUARD, DP, IP, sentinel, views, canon, plugin_path   # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 10
PLUGIN_IDS = {"lqr1d": 1001, "osc1d_exact_jacobian": 1005}
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "goddard_flow.json")))


def context(c, variant="exact"):
    from socp_amd import capi
    if c["model"] in PLUGIN_IDS:
        capi.plugin_load(plugin_path(c["model"]))
        ctx = capi.Context(PLUGIN_IDS[c["model"]], nparams=1)
    else:
        ctx = capi.Context({"goddard": capi.MODEL_GODDARD, "dint": capi.MODEL_DOUBLE_INTEGRATOR, "covid": capi.MODEL_COVID19}[c["model"]])
    ctx.set_variant(capi.VARIANT_LANE_FAST if variant == "fast" else capi.VARIANT_LANE_EXACT)
    ctx.set_params(c["params"])
    ctx.set_step_number(c["N"])
    if c.get("sw") is not None:
        ctx.set_switching_times(c["sw"])
    prob = c["prob"]
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    return ctx


# ---- the cases -----------------------------------------------------------------------------------------------------------------

def goddard_single():
    """M = 1 (n = 14), smooth law, 9 rows; row 4 starts from a NaN."""
    c = dict(jc.goddard_single(), N=N)
    Z = np.array(c["Z"])
    Z[4, 9] = np.nan
    return dict(c, Z=Z)


def goddard_m3():
    """M = 3, FREE tf (n = 43), smooth law; 9 rows = 27 groups: seven waves of four groups, the last with one idle group."""
    return dict(jc.goddard_m3(B=9, seed=9), N=N)


def goddard_m3_general():
    """The same structure with mu2 = 0: full thrust up to sw0 = 0.02, the closed-form singular control up to sw1 = 0.05 -- both
    switches fall inside a segment (the segments are about 0.03 long) -- then off; 3 rows."""
    c = goddard_m3()
    P = np.array(c["params"], dtype=np.float64)
    P[6] = 0.0
    assert P[7] < 0
    return dict(c, params=P, sw=(0.02, 0.05), Z=np.array(c["Z"][:3]))


def goddard_n87():
    """The free-switching-time structure of testGoddard's last stage (M = 6, n = 87: FREE nodes 2, 4 -- the model's switching times --
    and 6) at its golden solution, mu2 = 0; 2 rows."""
    from oracle.oracle import Problem, FREE
    from test_move_batch_cpu import stage4_structure, stage4_times
    z4 = np.array(GOLD["goddard_N10_M6"][3]["z"])
    z3 = np.array(GOLD["goddard_N10_M6"][2]["z"])
    mode_xf = np.zeros(7, dtype=np.int32)
    mode_xf[3:7] = FREE
    mode_t, mode_x = stage4_structure(mode_xf)
    X = np.zeros((7, 14))
    X[0, :7] = [0.999949994, 1e-4, 0.01, 1e-10, 1e-10, 1e-10, 1.0]
    X[6, 0] = 1.01
    Z = np.tile(z4, (2, 1))
    Z[1, :84] *= 1.0 + 1e-4
    prob = Problem(7, mode_t, mode_x, stage4_times(z3[-1]), X)
    assert prob.n == 87
    return dict(model="goddard", prob=prob, N=N, Z=Z, params=np.array([3.5, 7.0, 310.0, 500.0, 1.0, 1.0, 0.0, -1.0]))


def dint_fixed_node_free_tf():
    """M = 2 with a FIXED interior node (both sides pinned to xd) and a FREE tf; segment 1 saturates the control; 3 rows."""
    from oracle.oracle import Problem, FIXED, FREE
    n0 = np.array([0.0, 0.0, 0.0, 0.3, -0.2, 0.1, 0.02, -0.01, 0.015, 0.4, -0.3, 0.2])
    n1 = np.array([0.5, -0.3, 0.2, 0.1, 0.1, -0.2, 0.02, -0.01, 0.015, 2.0, -1.5, 1.0])
    Z = np.tile(np.concatenate([n0, n1, [3.0]]), (3, 1)) * (1.0 + 0.05 * np.random.default_rng(3).uniform(-1.0, 1.0, size=(3, 25)))
    mode_x = np.zeros((3, 6), dtype=np.int32)
    mode_x[2, 3:] = FREE
    X = np.zeros((3, 12))
    X[1, :6] = [0.45, -0.25, 0.2, 0.1, 0.1, -0.2]
    X[2, :3] = [1.0, -0.5, 0.3]
    prob = Problem(6, [FIXED, FIXED, FREE], mode_x, np.array([0.0, 1.5, 3.0]), X)
    return dict(model="dint", prob=prob, N=N, Z=Z, params=np.array([1.0, 1.0, 0.01]))


def dint_fixed_times():
    """M = 2, fixed times, CONTINUOUS interior node, the control unsaturated in both segments: the case of the cross-check against
    the variational equations, which (as the reference writes them, doubleIntegrator.cpp) do not differentiate the saturation -- on
    the saturated rows of dint_fixed_node_free_tf they differ from the derivative of the flow by 1.27 in entry (9, 21); 2 rows."""
    from oracle.oracle import Problem, FIXED, CONTINUOUS
    c = dint_fixed_node_free_tf()
    mode_x = np.zeros((3, 6), dtype=np.int32)
    mode_x[1] = CONTINUOUS
    prob = Problem(6, [FIXED, FIXED, FIXED], mode_x, c["prob"].time, c["prob"].xnode)
    Z = np.ascontiguousarray(c["Z"][:2, :24])
    Z[:, 21:24] *= 0.2                                                    # |u| = 0.54 at both nodes
    return dict(c, prob=prob, Z=Z)


def covid_m2():
    """M = 2, fixed times; node 0 with the control on its upper bound, node 1 with I >= Imax (the penalty); 3 rows."""
    from oracle.oracle import Oracle, Problem, MODEL_COVID, FIXED, CONTINUOUS
    o = Oracle(MODEL_COVID, step_nbr=N)
    n0 = np.array([0.9, 0.01, 0.05, 0.04, -1500.0, 300.0, 0.5, 0.1])
    n1 = np.array([0.6, 0.05, 0.2, 0.15, -0.5, 0.8, 0.3, 0.1])
    Z = np.tile(np.concatenate([n0, n1]), (3, 1)) * (1.0 + 0.02 * np.random.default_rng(4).uniform(-1.0, 1.0, size=(3, 16)))
    mode_x = np.zeros((3, 4), dtype=np.int32)
    mode_x[1] = CONTINUOUS
    prob = Problem(4, [FIXED, FIXED, FIXED], mode_x, np.array([0.0, 5.0, 10.0]), np.zeros((3, 8)))
    return dict(model="covid", prob=prob, N=N, Z=Z, params=o.params()[:8])


def osc1d_plugin():
    """tests/plugin/osc1d_exact_jacobian_plugin.hip, M = 2 with a FREE interior time and a FREE tf: its switching row reads X+; 5 rows
    = 10 groups of 3 lanes."""
    from oracle.oracle import Problem, FIXED, FREE, CONTINUOUS
    rng = np.random.default_rng(5)
    Z = np.hstack([rng.uniform(0.2, 1.0, size=(5, 4)), rng.uniform(0.8, 1.2, size=(5, 1)), rng.uniform(2.0, 2.5, size=(5, 1))])
    mode_x = np.zeros((3, 1), dtype=np.int32)
    mode_x[1] = CONTINUOUS
    prob = Problem(1, [FIXED, FREE, FREE], mode_x, np.array([0.0, 1.0, 2.0]), np.zeros((3, 2)))
    return dict(model="osc1d_exact_jacobian", prob=prob, N=N, Z=Z, params=np.array([4.0]))


CASES = {"goddard_single": goddard_single, "goddard_m3": goddard_m3, "goddard_m3_general": goddard_m3_general, "goddard_n87": goddard_n87,
         "dint_fixed_node_free_tf": dint_fixed_node_free_tf, "dint_fixed_times": dint_fixed_times, "covid_m2": covid_m2,
         "osc1d_plugin": osc1d_plugin}
_CASE, _REF = {}, {}


def case(name):
    if name not in _CASE:
        _CASE[name] = CASES[name]()
        _CASE[name]["Z"].setflags(write=False)
    return _CASE[name]


def reference_of(c, blocks=None, rows=None):
    model = "osc1d" if c["model"] == "osc1d_exact_jacobian" else c["model"]
    Z = c["Z"] if rows is None else c["Z"][rows]
    blocks = blocks if blocks is None or rows is None else tuple(a[rows] if a is not None else None for a in blocks)
    return ej.exact_jacobian_batch(model, [float(p) for p in c["params"]], c.get("sw") or (0.0, 0.0), c["prob"], Z, c["N"], blocks=blocks)


def reference(name):
    if name not in _REF:
        _REF[name] = reference_of(case(name))
    return _REF[name]


# ---- the forms on guarded buffers: each returns the two WHOLE buffers (Fjac, F) as integer views ----------------------------------

def run_host(ctx, Z, f=True, blocks=None):
    Z = np.ascontiguousarray(Z, dtype=np.float64)
    B, n = len(Z), ctx.n
    out = (sentinel(B * n * n), sentinel(B * n))
    tail = (out[0].ctypes.data_as(DP), out[1].ctypes.data_as(DP) if f else None)
    if blocks is None:
        ctx._chk(ctx.L.socp_exact_jacobian_batch(ctx.h, B, Z.ctypes.data_as(DP), *tail))
    else:
        pp, tt, xx = (np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in blocks)
        ptr = lambda a: a.ctypes.data_as(DP) if a is not None else None        # noqa: E731
        ctx._chk(ctx.L.socp_exact_jacobian_batch_blocks(ctx.h, B, Z.ctypes.data_as(DP), ptr(pp), pp.shape[1] if pp is not None else 0, ptr(tt),
                                                        ptr(xx), *tail))
    return views(out)


def run_dev(ctx, Z, f=True):
    import torch
    B, n = len(Z), ctx.n
    dZ = torch.from_numpy(np.array(Z, dtype=np.float64)).cuda()
    dev = [torch.from_numpy(a).cuda() for a in (sentinel(B * n * n), sentinel(B * n))]
    torch.cuda.synchronize()
    ctx.exact_jacobian_batch_dev(B, dZ.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr() if f else None)
    ctx.synchronize()
    torch.cuda.synchronize()
    return views(tuple(t.cpu().numpy() for t in dev))


def check_whole(got, want, what):
    for name, g, w in zip(("Fjac", "F"), got, want):
        if w is None:
            assert np.all(g == np.uint64(SENT)), "%s: %s was written although its pointer was NULL" % (what, name)
            continue
        w = np.ascontiguousarray(w, dtype=np.float64).ravel().view(np.uint64)
        assert np.all(g[w.size:] == np.uint64(SENT)), "%s: guard words behind %s were written" % (what, name)
        gg, ww = canon(g[:w.size]), canon(w)
        bad = np.argwhere(gg != ww).ravel()
        assert len(bad) == 0, (what, name, "%d differ; first flat indices:" % len(bad), bad[:5].tolist(), gg[bad[:5]].view(np.float64),
                               ww[bad[:5]].view(np.float64))


def matrices(view, B, n):
    """J[b][row][col] of a whole Fjac buffer."""
    return view[:B * n * n].view(np.float64).reshape(B, n, n).transpose(0, 2, 1)


# ---- 1. every case, host and _dev forms, bit for bit -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement(name):
    c = case(name)
    want = reference(name)
    ctx = context(c)
    assert ctx.has_exact_jacobian()
    t0, l0 = ctx.counters()
    check_whole(run_host(ctx, c["Z"]), want, name + ", host form")
    check_whole(run_dev(ctx, c["Z"]), want, name + ", _dev form")
    t1, l1 = ctx.counters()
    B, M, S = len(c["Z"]), c["prob"].M, 2 * c["prob"].dim
    assert t1 - t0 == 2 * B * M * (S + 1) and l1 - l0 == 2, "B M (S + 1) trajectories and one launch per call"
    check_whole(run_dev(ctx, c["Z"], f=False), (want[0], None), name + ", NULL F")
    # F is socp_residual_batch of this reference-order context, bit for bit
    F = ctx.residual_batch(np.ascontiguousarray(c["Z"]))
    assert np.array_equal(canon(F.view(np.uint64)), canon(np.ascontiguousarray(want[1]).view(np.uint64))), "F against socp_residual_batch"
    if name == "goddard_single":
        J = want[0].reshape(9, 14, 14)
        assert not np.isfinite(J[4]).all() and np.isfinite(np.delete(J, 4, axis=0)).all(), "the NaN row and only it"
        check_whole(run_dev(ctx, c["Z"][:1]), (want[0][:1], want[1][:1]), "B = 1")
    if name == "goddard_m3":
        check_whole(run_dev(ctx, c["Z"][:1]), (want[0][:1], want[1][:1]), "B = 1")
        J = want[0].reshape(9, 43, 43).transpose(0, 2, 1)
        assert all(np.abs(J[:, rows, 42]).max() > 0 for rows in (slice(14, 28), slice(28, 42), slice(7, 14))), "the free-time column is filled"
    if name == "goddard_m3_general":
        smooth = reference_of(dict(case("goddard_m3"), Z=c["Z"]), rows=[0])
        assert not np.array_equal(smooth[0][0], want[0][0]), "the launch took the general-law kernel"
    ctx.close()


# ---- 2. per-row blocks -----------------------------------------------------------------------------------------------------------

def test_blocks_form_and_each_row_alone():
    from oracle.oracle import Problem
    c = case("goddard_m3")
    B, prob = len(c["Z"]), c["prob"]
    ctx = context(c)
    plain = run_host(ctx, c["Z"])
    params = np.tile(np.concatenate([c["params"], [0.0, 0.0]]), (B, 1))
    params[:, 2] = np.linspace(250.0, 330.0, B)                           # KD
    params[:, 6] = np.linspace(0.5, 1.5, B)                               # mu2 > 0 in every row
    xnode = np.tile(prob.xnode.ravel(), (B, 1))
    xnode[:, 3 * 14] = np.linspace(1.005, 1.015, B)                       # the final altitude
    time = np.tile(prob.time, (B, 1))
    time[:, 0] = np.linspace(0.0, 0.008, B)                               # t0 (FIXED): every node time of the row moves with it
    want = reference_of(c, blocks=(params, time, xnode))
    got = run_host(ctx, c["Z"], blocks=(params, time, xnode))
    check_whole(got, want, "_blocks form")
    assert not np.array_equal(got[0], plain[0])
    only_time = run_host(ctx, c["Z"], blocks=(None, time, None))
    check_whole(only_time, reference_of(c, blocks=(None, time, None)), "_blocks form, the time block alone")
    n = prob.n
    assert np.array_equal(only_time[0][:n * n], plain[0][:n * n]) and not np.array_equal(only_time[0][n * n:2 * n * n], plain[0][n * n:2 * n * n])
    again = run_host(ctx, c["Z"])
    assert all(np.array_equal(a, b) for a, b in zip(plain, again)), "the context's own blocks are back"
    for b in range(B):                                                    # EACH row equals the row run alone
        one = dict(c, params=params[b, :8], prob=Problem(7, prob.mode_t, prob.mode_x, time[b], xnode[b]))
        cb = context(one)
        row = run_host(cb, c["Z"][b:b + 1])
        cb.close()
        assert np.array_equal(canon(got[0][b * n * n:(b + 1) * n * n]), canon(row[0][:n * n])), b
        assert np.array_equal(canon(got[1][b * n:(b + 1) * n]), canon(row[1][:n])), b
    ctx.close()


# ---- 3. the throughput flavour ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard_m3", "goddard_m3_general", "covid_m2"])
def test_throughput_flavour_returns_the_same_bits(name):
    c = case(name)
    ctx = context(c, "fast")
    assert ctx.has_exact_jacobian()
    check_whole(run_dev(ctx, c["Z"]), reference(name), name + ", throughput flavour")
    ctx.close()


# ---- 4. cross-checks ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["goddard_m3", "goddard_m3_general", "dint_fixed_times", "covid_m2"])
def test_continuity_block_is_phi_of_fields_batch(name):
    """Cross-check 1: rows S (i + 1) .., columns S i .. of every interior node equal Phi of socp_fields_batch (SOCP_FIELDS_ALL) as numbers."""
    c = case(name)
    ctx = context(c)
    Z = c["Z"]
    B, M, S, n = len(Z), c["prob"].M, 2 * c["prob"].dim, c["prob"].n
    J = matrices(run_dev(ctx, Z)[0], B, n)
    phi = ctx.fields_batch(Z, cols=fr.ALL, stride=N, cap=4, phi=True)["phi"].cpu().numpy()
    assert np.isfinite(phi).all()
    for i in range(M - 1):
        assert np.array_equal(J[:, S * (i + 1):S * (i + 2), S * i:S * (i + 1)], phi[:, i]), (name, i)
    ctx.close()


def test_state_columns_agree_with_the_variational_jacobian():
    """Cross-check 2: RK4 on the variational system IS the derivative of the RK4 flow, so on the double integrator with fixed times the
    two Jacobians agree at rounding level.  Bound: 8 x the deviation of the CPU restatement from the same recurrence in 240 bits."""
    import torch
    c = case("dint_fixed_times")
    ctx = context(c)
    Z = np.array(c["Z"])
    B, n = Z.shape
    J = matrices(run_dev(ctx, Z)[0], B, n)
    dZ = torch.from_numpy(Z).cuda()
    dJ = torch.zeros((B, n, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx._chk(ctx.L.socp_var_jacobian_multi_dev(ctx.h, B, dZ.data_ptr(), dJ.data_ptr()))
    ctx.synchronize()
    Jvar = dJ.cpu().numpy().transpose(0, 2, 1)
    if fr.HAVE_MPMATH:
        truth, _ = ej.exact_jacobian_row("dint", c["params"], (0.0, 0.0), c["prob"], Z[0], N, high=True)
        own = float(max(abs(fr.mpf(float(a)) - q) for a, q in zip(J[0].ravel(), truth.ravel())))
    else:
        own = 16 * 2.0 ** -53 * np.abs(J[0]).max()
    dev = float(np.abs(J[0] - Jvar[0]).max())
    print("dint, fixed times: |J_exact - J_var| %.3e; the restatement's own deviation from the 240-bit recurrence %.3e; ratio %.3f"
          % (dev, own, dev / own if own else float("nan")))
    assert own > 0 and dev <= 8 * own
    ctx.close()


# ---- 5. one use ----------------------------------------------------------------------------------------------------------------

def test_svd_and_linsolve_take_the_output_and_a_newton_step_lowers_the_residual():
    import torch
    from conftest import goddard_single_problem
    prob, zstar = goddard_single_problem()
    c = dict(model="goddard", prob=prob, N=100, params=case("goddard_single")["params"])
    ctx = context(c)
    z0 = ctx.multistart_solve(zstar[None, :])["z"]                         # the root at this step number
    Z = np.tile(z0, (3, 1))
    Z[:, 7:] *= 1.0 + 1e-5 * np.random.default_rng(6).uniform(-1.0, 1.0, size=(3, 7))
    n = 14
    J, F = ctx.exact_jacobian_batch(Z, residual=True)
    sigma = torch.zeros((3, n), dtype=torch.float64, device="cuda")
    sweeps, info = (torch.zeros(3, dtype=torch.int32, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    keep = J.clone()
    ctx.svd_batch_dev(3, n, J.data_ptr(), 60, sigma.data_ptr(), None, sweeps.data_ptr(), info.data_ptr())
    ctx.synchronize()
    assert torch.equal(J, keep) and int(info.abs().sum()) == 0
    s_np = np.linalg.svd(J.cpu().numpy().transpose(0, 2, 1), compute_uv=False)
    assert np.allclose(sigma.cpu().numpy(), s_np, rtol=1e-9, atol=1e-12 * s_np.max())
    Y = (-F).clone().reshape(3, 1, n).contiguous()
    linfo = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.linsolve_batch_dev(3, n, 1, J.data_ptr(), Y.data_ptr(), linfo.data_ptr())
    ctx.synchronize()
    assert int(linfo.abs().sum()) == 0
    Z1 = Z + Y.reshape(3, n).cpu().numpy()
    before, after = np.abs(ctx.residual_batch(Z)).max(axis=1), np.abs(ctx.residual_batch(Z1)).max(axis=1)
    print("one Newton correction from the exact Jacobian: |F|inf %s -> %s" % (before, after))
    assert np.all(after < before)
    ctx.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------

def raw(ctx, B, Z, out, form="host"):
    fn = ctx.L.socp_exact_jacobian_batch if form == "host" else ctx.L.socp_exact_jacobian_batch_dev
    ptr = (lambda a: a.ctypes.data_as(DP) if a is not None else None) if form == "host" else (lambda a: a.ctypes.data if a is not None else None)
    return fn(ctx.h, B, ptr(Z), ptr(out[0]), ptr(out[1]))


def test_refusals_write_nothing_and_carry_a_message():
    from socp_amd import capi
    from oracle.oracle import Problem, FREE
    c = case("goddard_m3")
    ctx = context(c)
    Z = np.ascontiguousarray(c["Z"])
    B, n = Z.shape
    out = (sentinel(B * n * n), sentinel(B * n))
    fresh_out = lambda o: all(np.all(v == np.uint64(SENT)) for v in views(o))      # noqa: E731
    L, h = ctx.L, ctx.h
    t0 = ctx.counters()
    assert raw(ctx, -1, Z, out) == capi.ERR_ARG and "B >= 0" in L.socp_last_error(h).decode()
    for form in ("host", "dev"):
        assert raw(ctx, B, None, out, form) == capi.ERR_ARG and raw(ctx, B, Z, (None, out[1]), form) == capi.ERR_ARG
        assert raw(ctx, 0, None, (None, None), form) == capi.OK
    params = np.tile(np.concatenate([ctx.get_params(), [0.0, 0.0]]), (B, 1))
    for pstride in (8, 9, 11):
        assert L.socp_exact_jacobian_batch_blocks(h, B, Z.ctypes.data_as(DP), params.ctypes.data_as(DP), pstride, None, None,
                                                  out[0].ctypes.data_as(DP), None) == capi.ERR_ARG, pstride
    assert "nparams + 2" in L.socp_last_error(h).decode()
    ctx.set_integrator(capi.INT_DOPRI5, 1e-8)
    for form in ("host", "dev"):
        assert raw(ctx, B, Z, out, form) == capi.ERR_UNSUPPORTED and "DOPRI5" in L.socp_last_error(h).decode()
    ctx.set_integrator(capi.INT_RK4)
    # a FREE state component on an interior node
    prob = c["prob"]
    mode_x = prob.mode_x.copy()
    mode_x[1, 2] = FREE
    assert ctx.problem_set(prob.mode_t, mode_x, prob.time, prob.xnode) == prob.n
    for form in ("host", "dev"):
        assert raw(ctx, B, Z, out, form) == capi.ERR_UNSUPPORTED and "FREE state component" in L.socp_last_error(h).decode()
    assert ctx.problem_set(prob.mode_t, prob.mode_x, prob.time, prob.xnode) == prob.n
    assert ctx.counters() == t0 and fresh_out(out), "nothing was launched, counted or written"
    fresh = capi.Context(capi.MODEL_GODDARD)
    assert fresh.has_exact_jacobian()
    assert raw(fresh, B, Z, out) == capi.ERR_ARG and "no problem set" in fresh.L.socp_last_error(fresh.h).decode()
    fresh.close()

    # models without the entry: the interceptor, vtolUAV and lqr1d (no traits)
    from test_gpu_interceptor import multi_shooting_problem, scenario_state
    from test_gpu_cost_batch import build_vtol
    from oracle.oracle import Oracle, MODEL_INTERCEPTOR
    Xs, Xf = scenario_state(gamma=1.49)
    iprob, iz = multi_shooting_problem(Oracle(MODEL_INTERCEPTOR), 4, X0=Xs, Xf=Xf)
    ci = capi.Context(capi.MODEL_INTERCEPTOR)
    assert ci.problem_set(iprob.mode_t, iprob.mode_x, iprob.time, iprob.xnode) == iprob.n
    assert not ci.has_exact_jacobian() and ci.L.socp_ctx_has_exact_jacobian(ci.h) == 0
    io = (sentinel(iprob.n * iprob.n), sentinel(iprob.n))
    c0 = ci.counters()
    assert raw(ci, 1, np.ascontiguousarray(iz), io) == capi.ERR_UNSUPPORTED
    assert "no exact_jacobian entry" in ci.L.socp_last_error(ci.h).decode() and ci.counters() == c0 and fresh_out(io)
    with pytest.raises(capi.SocpError):
        ci.exact_jacobian_batch(iz[None, :])
    ci.close()
    cv, _, Zv, _ = build_vtol("exact")
    assert not cv.has_exact_jacobian()
    vo = (sentinel(len(Zv) * cv.n * cv.n), sentinel(len(Zv) * cv.n))
    assert raw(cv, len(Zv), np.ascontiguousarray(Zv), vo) == capi.ERR_UNSUPPORTED and fresh_out(vo)
    assert "no exact_jacobian entry" in cv.L.socp_last_error(cv.h).decode()
    cv.close()
    lq = jc.case("lqr1d")
    cl = context(dict(lq))
    assert not cl.has_exact_jacobian() and cl.has_jacobi()
    lo = (sentinel(len(lq["Z"]) * cl.n * cl.n), sentinel(len(lq["Z"]) * cl.n))
    assert raw(cl, len(lq["Z"]), np.ascontiguousarray(lq["Z"]), lo) == capi.ERR_UNSUPPORTED and fresh_out(lo)
    assert "no exact_jacobian entry" in cl.L.socp_last_error(cl.h).decode()
    cl.close()
    for model in (capi.MODEL_GODDARD, capi.MODEL_DOUBLE_INTEGRATOR, capi.MODEL_COVID19):
        for variant in (capi.VARIANT_LANE_EXACT, capi.VARIANT_LANE_FAST):
            cm = capi.Context(model)
            cm.set_variant(variant)
            assert cm.has_exact_jacobian()
            cm.close()

    # a valid call afterwards: the bits of the restatement
    check_whole(run_host(ctx, Z), reference("goddard_m3"), "after the refused calls")
    ctx.close()


# ---- 6b. the sweep tool's forward difference is the context's own ---------------------------------------------------------------

@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_sweep_fd_dev_differences_the_residual_of_the_contexts_flavour(variant, tmp_path):
    """exactjac_local's fd_dev against the same figure formed here from socp_residual_batch_dev + socp_fd_jacobian_multi_dev of THIS
    context: equal in both flavours.  (With the exact call's F, the reference-order residual, as the base of a throughput-flavour
    difference the flavours' gap would be divided by the step.)"""
    import argparse
    import torch
    from socp_amd import sweep
    c = case("goddard_single")
    ctx = context(dict(c, N=100), variant)
    Z = np.delete(np.array(c["Z"]), 4, axis=0)                            # without the NaN row
    B, n = Z.shape
    local = dict(info=np.ones(B, dtype=np.int32), z=Z)
    entry = sweep.exactjac_local(ctx, argparse.Namespace(exactjac_out=str(tmp_path / "ej")), local, 0, 0)
    got = np.load(entry["file"])["fd_dev"]
    dZ = torch.from_numpy(Z).cuda()
    dF = torch.empty((B, n), dtype=torch.float64, device="cuda")
    dJfd = torch.empty((B, n, n), dtype=torch.float64, device="cuda")
    J = ctx.exact_jacobian_batch(dZ)
    torch.cuda.synchronize()
    ctx.residual_batch_dev(B, dZ.data_ptr(), dF.data_ptr())
    ctx.fd_jacobian_multi_dev(B, dZ.data_ptr(), dF.data_ptr(), 1e-15, dJfd.data_ptr())
    ctx.synchronize()
    want = ((dJfd - J).abs().amax(dim=(1, 2)) / J.abs().amax(dim=(1, 2))).cpu().numpy()
    print("fd_dev of 8 nominal Goddard rows, N = 100, %s flavour: median %.3e, max %.3e" % (variant, np.median(got), got.max()))
    assert np.array_equal(got, want)
    ctx.close()


# ---- 7. the sweep tool -----------------------------------------------------------------------------------------------------------

def test_sweep_tool_writes_the_exact_jacobian_file_and_record(tmp_path):
    out = str(tmp_path / "ej")
    run = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--starts", "64", "--rk4-steps", "50", "--exactjac-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    entry = rec["exact_jacobian"]
    assert {"rows", "fd_dev_median", "fd_dev_max", "sigma_min_min"} <= set(entry)
    npz = np.load(entry["file"])
    assert entry["file"] == out + ".rank0.npz" and sorted(npz.files) == ["fd_dev", "index", "sigma"]
    k = entry["rows"]
    assert k == rec["converged"] == len(npz["index"]) > 0
    assert npz["fd_dev"].shape == (k,) and npz["sigma"].shape == (k, 14)
    assert entry["fd_dev_max"] == float(npz["fd_dev"].max()) >= entry["fd_dev_median"] > 0
    assert entry["sigma_min_min"] == float(npz["sigma"][:, -1].min()) >= 0
    print("sweep --exactjac-out, 64 starts: %s" % {q: entry[q] for q in ("rows", "fd_dev_median", "fd_dev_max", "sigma_min_min")})
    bad = subprocess.run([sys.executable, "-m", "socp_amd.sweep", "--model", "interceptor", "--exactjac-out", out], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--exactjac-out" in bad.stderr
